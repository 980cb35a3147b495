// rmp2_hip.hip -- the C ABI of the MI355X RMP2 engine (include/rmp2.h), the program compiler, the kernel
// dispatch and the lane-per-robot kernels.
//
// One control step = ONE kernel launch: forward kinematics -> per-frame Jacobian columns and J-dot-qd ->
// leaf (xdd, A) evaluation -> pull-back J^T A J / J^T A (xdd - c) -> sum over leaves (fp64) ->
// resolve (fp64 elimination, pseudo-inverse fall-through) -> qdd.  Algorithmic HBM traffic per robot
// and step: q, qd in, qdd out (+ goal): 120 B for the Panda.  Which kernel runs a step is decided
// by fleet size in dispatch_solve(): rmp2_hex.h (<= 8192 robots), rmp2_quad.h, or rmp2_step_kernel below.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>

#include <chrono>

#include <map>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "rmp2_host.h"
#include "rmp2_hull.h"
#include "rmp2_dynamics.h"
#include "rmp2_forward_dynamics.h"
#include "rmp2_joint_stops.h"
#include "rmp2_contacts.h"
#include "rmp2_stages.h"  // the geometry stage kernels (FK, closest points, self pairs, hulls, FK differentiation)

using namespace rmp2;

namespace {

// =========================================================================================
// device: the fused control-step kernel
// =========================================================================================
// LDS layout per 64-robot block (floats):
//   [0, 64*N)            q tile, robot-major (row r = lane r)   -- coalesced global load,
//   [64*N, 128*N)        qd tile                                  stride-N lane reads: N odd -> no conflicts
//   [128*N, 128*N+6*N*64) per-dof world axis z_j and joint origin o_j, component-major
//                         ((j*6+c)*64 + lane): lane-private columns, conflict free
//   [.., +64*N)           qdd tile (written right after the resolve, stored coalesced at the end)
template <int N>
struct Lds {
  static constexpr int kQ = 0;
  static constexpr int kQd = kWave * N;
  static constexpr int kZo = 2 * kWave * N;
  static constexpr int kOut = 2 * kWave * N + 6 * N * kWave;  // qdd tile, robot-major (stride n_dof)
  static constexpr int kFloats = 3 * kWave * N + 6 * N * kWave;
};

// Jacobian columns of a point pt moving with a frame: z_j x (pt - o_j) (revolute ancestors), z_j (prismatic),
// 0 for joints that do not move the frame.  zo = this lane's column of the LDS z/o table.
template <int N>
__device__ __forceinline__ void fill_cols(float (&col)[N][3], const float* zo, uint32_t anc_mask, uint32_t rev_mask,
                                          const float pt[3], const float origin[3]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if ((anc_mask >> j) & 1u) {
      const float zj[3] = {zo[(j * 6 + 0) * kWave], zo[(j * 6 + 1) * kWave], zo[(j * 6 + 2) * kWave]};
      if ((rev_mask >> j) & 1u) {
        // (bit 16 + j: the frame's origin lies on joint j's axis for every q -- structural_lever_zeros: it is the axis point)
        const bool on_axis = (anc_mask >> (16 + j)) & 1u;
        const float d[3] = {pt[0] - (on_axis ? origin[0] : zo[(j * 6 + 3) * kWave]), pt[1] - (on_axis ? origin[1] : zo[(j * 6 + 4) * kWave]),
                            pt[2] - (on_axis ? origin[2] : zo[(j * 6 + 5) * kWave])};
        cross3(zj, d, col[j]);
      } else {
        col[j][0] = zj[0];
        col[j][1] = zj[1];
        col[j][2] = zj[2];
      }
    } else {
      col[j][0] = col[j][1] = col[j][2] = 0.f;
    }
  }
}

// EXT = build with the rarely used extensions (attached-point leaves, capsule primitives); the EXT = false
// build is the hot one and carries none of their code.
template <int N, int SLOTS, bool STRICT, bool EXT>
__global__ void __launch_bounds__(kWave)
rmp2_step_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ q, const float* __restrict__ qd,
                 const float* __restrict__ goal, int goal_stride, ObsArgs obs, OutArgs out, int R) {
  __shared__ float lds[Lds<N>::kFloats];
  const int lane = threadIdx.x;
  const int r0 = blockIdx.x * kWave;
  const int robot = r0 + lane;
  const bool live = robot < R;
  const int n_dof = prog->n_dof;

  // ---- coalesced load of the q / qd tile (contiguous n_dof*64 floats), zero padded --------
  {
    const int tile = min(kWave, R - r0) * n_dof;
    const float* gq = q + (size_t)r0 * n_dof;
    const float* gqd = qd + (size_t)r0 * n_dof;
    for (int i = lane; i < kWave * N; i += kWave) {
      lds[Lds<N>::kQ + i] = 0.f;
      lds[Lds<N>::kQd + i] = 0.f;
    }
    __syncthreads();
    for (int i = lane; i < tile; i += kWave) {
      const int rr = i / n_dof, jj = i - rr * n_dof;
      lds[Lds<N>::kQ + rr * N + jj] = gq[i];
      lds[Lds<N>::kQd + rr * N + jj] = gqd[i];
    }
    __syncthreads();
  }
  const float* my_q = &lds[Lds<N>::kQ + lane * N];
  const float* my_qd = &lds[Lds<N>::kQd + lane * N];
  float* zo = &lds[Lds<N>::kZo + lane];
  const float* my_goal = goal ? goal + (size_t)(live ? robot : 0) * goal_stride : nullptr;
  const uint32_t rev_mask = prog->rev_mask;

  float* my_out = &lds[Lds<N>::kOut + lane * n_dof];
  uint32_t status = 0u;
  bool singular = false;

  // AUTO build (STRICT = false): pass 0 = accumulate + fp64 LU.  Only when some lane of the
  // wave turns out (numerically) singular a second pass re-accumulates and resolves those
  // lanes with the compact pseudo-inverse (rare path, scratch memory, deliberately not
  // unrolled so that it costs the common path no registers and ~no code).
  // STRICT build (solve_mode = PINV): one pass, register-resident Jacobi pseudo-inverse.
#pragma nounroll
  for (int pass = STRICT ? 1 : 0; pass < 2; ++pass) {
    double Ms[N * (N + 1) / 2];  // upper triangle of the FK-leaf part (always symmetric)
    double fv[N];
#pragma unroll
    for (int i = 0; i < N * (N + 1) / 2; ++i) Ms[i] = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) fv[i] = 0.0;

    // ---- walk the kinematic tree -------------------------------------------------------
    FrameState cur;
    FrameState slot[SLOTS > 0 ? SLOTS : 1];
    const int n_ops = prog->n_ops;
    for (int k = 0; k < n_ops; ++k) {
      const DevOp& op = prog->ops[k];
      if (SLOTS > 0 && op.restore >= 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
          if (op.restore == s) cur = slot[s];
      }
      const int qi = op.qidx;
      const float qv = qi >= 0 ? my_q[qi] : 0.f;
      const float qdv = qi >= 0 ? my_qd[qi] : 0.f;
      float z[3];
      visit_frame<true>(cur, op, qv, qdv, op.restore == -2, z);
      if (qi >= 0 && op.jtype != RMP2_JOINT_FIXED) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          zo[(qi * 6 + c) * kWave] = z[c];
          zo[(qi * 6 + 3 + c) * kWave] = cur.p[c];
        }
      }
      if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
          if (op.save == s) slot[s] = cur;
      }
      if (op.leaf_count == 0) continue;

      // Jacobian columns of this frame's origin: z_j x (p - o_j) (revolute) or z_j (prismatic)
      float col[N][3];
      fill_cols<N>(col, zo, op.anc_mask, rev_mask, cur.p, cur.p);

      for (int li = 0; li < op.leaf_count; ++li) {
        const DevLeaf& lf = prog->leaves[prog->fk_leaves[op.leaf_begin + li]];
        // attached-point leaves (taskmap.py:79-99 chain) pull every pair back through its own Jacobian:
        // one trip of the block below per pair; all other leaves take exactly one trip
        const bool point = EXT && lf.taskmap == RMP2_TASKMAP_FK_POINT;
        int trips = 1;
        size_t pbase = 0;
        if (EXT && point) {
          const int pb = obs.pair_begin[lf.index];
          trips = obs.pair_begin[lf.index + 1] - pb;
          pbase = (size_t)(live ? robot : 0) * obs.n_pairs + pb;
        }
#pragma nounroll
        for (int trip = 0; trip < trips; ++trip) {
        float S[6], h[3];
        if (lf.taskmap == RMP2_TASKMAP_FK_POSITION) {
          // chain [FK(frame), 4x4 -> position]: x = p, xd = v, c = a_bias (taskmap.py:150-160)
          float g[3], xdd[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) g[c] = my_goal[lf.goal_offset + c];
          if (lf.kind == RMP2_LEAF_TARGET_ATTRACTOR)
            leaf_target_attractor(lf.P, cur.p, cur.v, g, xdd, S);
          else
            leaf_target_policy3(lf.P, cur.p, cur.v, g, xdd, S);
          const float e[3] = {xdd[0] - cur.a[0], xdd[1] - cur.a[1], xdd[2] - cur.a[2]};
          h[0] = S[0] * e[0] + S[1] * e[1] + S[2] * e[2];
          h[1] = S[1] * e[0] + S[3] * e[1] + S[4] * e[2];
          h[2] = S[2] * e[0] + S[4] * e[1] + S[5] * e[2];
        } else if (EXT && point) {
          // chain [FK(frame), TaskmapRelative4x4(rel), 4x4 -> position] for pair `trip`:
          //   r = R rel, x = p + r, xd = v + w x r, c = a + al x r + w x (w x r), J = Jacobian at x
          const float* rel = obs.p_link + (pbase + trip) * 3;
          const float* nvp = obs.p_obs + (pbase + trip) * 3;
          const float dd = obs.dist[pbase + trip];
          float r[3], pt[3], t1[3], t2[3], xdp[3], cp[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            r[c] = cur.R[3 * c] * rel[0] + cur.R[3 * c + 1] * rel[1] + cur.R[3 * c + 2] * rel[2];
            pt[c] = cur.p[c] + r[c];
          }
          cross3(cur.w, r, t1);
#pragma unroll
          for (int c = 0; c < 3; ++c) xdp[c] = cur.v[c] + t1[c];
          cross3(cur.w, t1, t2);
          cross3(cur.al, r, t1);
#pragma unroll
          for (int c = 0; c < 3; ++c) cp[c] = cur.a[c] + t1[c] + t2[c];
          fill_cols<N>(col, zo, op.anc_mask, rev_mask, pt, cur.p);
          const float nv[3] = {nvp[0], nvp[1], nvp[2]};
          float xdd[3], wgt;
          leaf_collision_avoidance(lf.P, dd, nv, xdp, xdd, wgt);
          S[0] = S[3] = S[5] = wgt;
          S[1] = S[2] = S[4] = 0.f;
#pragma unroll
          for (int c = 0; c < 3; ++c) h[c] = wgt * (xdd[c] - cp[c]);
        } else {
          // chain [FK(frame), 4x4 -> distance] over this leaf's pairs.  Every pair pulls back
          // through the SAME 3 x n Jacobian, so the per-pair rank-1 updates collapse into
          //   S = sum_b a_b n_b n_b^T ,  h = sum_b a_b (xdd_b - c_b) n_b     (fp32, like the
          // reference's reduce_sum over the pair axis, rmp.py:149-150)
#pragma unroll
          for (int c = 0; c < 6; ++c) S[c] = 0.f;
          h[0] = h[1] = h[2] = 0.f;
          const float vv = dot3(cur.v, cur.v);
          int count;
          const float* pl = nullptr;
          const float* po = nullptr;
          const int32_t* ci = nullptr;
          if (obs.mode == RMP2_OBS_EXPLICIT_PAIRS) {
            const int pb = obs.pair_begin[lf.index];
            count = obs.pair_begin[lf.index + 1] - pb;
            const size_t base = ((size_t)(live ? robot : 0) * obs.n_pairs + pb) * 3;
            pl = obs.p_link + base;
            po = obs.p_obs + base;
          } else if (obs.mode == RMP2_OBS_SHARED_SPHERES) {
            count = obs.n_spheres;
          } else {
            const int b0 = obs.csr_offset[live ? robot : 0];
            count = live ? obs.csr_offset[robot + 1] - b0 : 0;
            ci = obs.csr_index + b0;
          }
          const bool uniform_count = obs.mode != RMP2_OBS_RAGGED_SPHERES;
          int max_count = count;
          if (!uniform_count) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) max_count = max(max_count, __shfl_xor(max_count, o));
          }
          for (int b = 0; b < max_count; ++b) {
            float diff[3], nh[3], d;
            bool on = true;
            if (obs.mode == RMP2_OBS_EXPLICIT_PAIRS) {
              // taskmap.py:124-129: rel = stop_gradient(p_link - p_joint); crit = p_joint + rel
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                const float rel = pl[3 * b + c] - cur.p[c];
                const float crit = cur.p[c] + rel;
                diff[c] = crit - po[3 * b + c];
              }
              d = sqrtf(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]);
#pragma unroll
              for (int c = 0; c < 3; ++c) nh[c] = diff[c] / d;
            } else {
              int sidx = b;
              if (!uniform_count) {
                on = b < count;
                sidx = on ? ci[b] : 0;
              }
              float4 sp;
              float ctr[3];
              if (EXT && obs.cylinder) {  // finite cylinder: nearest surface point, outward normal, signed distance
                float Yc[3];
                point_cylinder(reinterpret_cast<const float4*>(obs.spheres)[2 * sidx], reinterpret_cast<const float4*>(obs.spheres)[2 * sidx + 1],
                               cur.p, Yc, nh, d);
              } else {
              if (EXT && obs.capsule) {
                sp = reinterpret_cast<const float4*>(obs.spheres)[2 * sidx];
                capsule_centre(sp, reinterpret_cast<const float4*>(obs.spheres)[2 * sidx + 1], cur.p, ctr);
              } else {
                sp = reinterpret_cast<const float4*>(obs.spheres)[sidx];
                ctr[0] = sp.x, ctr[1] = sp.y, ctr[2] = sp.z;
              }
              diff[0] = cur.p[0] - ctr[0];
              diff[1] = cur.p[1] - ctr[1];
              diff[2] = cur.p[2] - ctr[2];
              const float dc = sqrtf(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]);
              d = dc - sp.w;
#pragma unroll
              for (int c = 0; c < 3; ++c) nh[c] = diff[c] / dc;
              }
            }
            const float xdot = dot3(nh, cur.v);
            const float cd = (vv - xdot * xdot) / d + dot3(nh, cur.a);  // c2 + J2 c1 (taskmap.py:159)
            float acc, met;
            leaf_obstacle_avoidance(lf.P, d, xdot, acc, met);
            if (!on) met = 0.f;
            const float wgt = met * (acc - cd);
            const float mn[3] = {met * nh[0], met * nh[1], met * nh[2]};
            S[0] += mn[0] * nh[0];
            S[1] += mn[0] * nh[1];
            S[2] += mn[0] * nh[2];
            S[3] += mn[1] * nh[1];
            S[4] += mn[1] * nh[2];
            S[5] += mn[2] * nh[2];
            h[0] += wgt * nh[0];
            h[1] += wgt * nh[1];
            h[2] += wgt * nh[2];
          }
        }
        pull_position<N>(col, op.anc_mask, S, h, Ms, fv);
        }  // trip
        if (EXT && point) fill_cols<N>(col, zo, op.anc_mask, rev_mask, cur.p, cur.p);
      }
    }

    // ---- identity-task-map leaves: x = q, xd = qd, J = I, c = 0 (taskmap.py:13-20) ----------
    double A[N][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < N; ++j) A[i][j] = Ms[sym_idx<N>(i < j ? i : j, i < j ? j : i)];
    // q / qd are re-read from the LDS tile where needed (keeps them out of the VGPR budget
    // while the 81 fp64 accumulators are live)
#define ql my_q
#define qdl my_qd
    const int n_id = prog->n_id_leaves;
    for (int li = 0; li < n_id; ++li) {
      const DevLeaf& lf = prog->leaves[prog->id_leaves[li]];
      const float* __restrict__ P = lf.P;
      float xdd[N];
      if (lf.kind == RMP2_LEAF_JOINT_DAMPING) {
        // rmp2.py:127-137
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) s2 += qdl[i] * qdl[i];
        const float nrm = sqrtf(s2);
        const float m = P[1] * nrm + P[2];
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const float acc = -(P[0] * nrm) * qdl[i];
          A[i][i] += (double)m;
          fv[i] += (double)(m * acc);
        }
      } else if (lf.kind == RMP2_LEAF_CSPACE_BIASING) {
        // rmp2.py:212-226
        float e[N], s2 = 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          e[i] = ql[i] - lf.va[i];
          s2 += e[i] * e[i];
        }
        const float en = sqrtf(s2);
        const float m = P[0] + P[4];
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const float pos = (en < P[3]) ? (-e[i] * P[1]) : (-P[3] * (e[i] / en) * P[1]);
          const float acc = pos + (-P[2] * qdl[i]);
          A[i][i] += (double)m;
          fv[i] += (double)(m * acc);
        }
      } else if (lf.kind == RMP2_LEAF_CONFIG_SPACE_BIASING) {
        // rmp.py:330-347
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const float acc = P[0] * (lf.va[i] - ql[i]) - P[1] * qdl[i];
          A[i][i] += (double)P[2];
          fv[i] += (double)(P[2] * acc);
        }
      } else if (lf.kind == RMP2_LEAF_JOINT_VELOCITY_CAP) {
        // rmp2.py:100-112; metric = w / (1 - diag(ratio^2)) on the FULL matrix (quirk Q4)
        const float cutoff = P[0] - P[1];
        float dg[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const float dv = fabsf(qdl[i]) - cutoff;
          const float sgn = (qdl[i] > 0.f) ? 1.f : (qdl[i] < 0.f ? -1.f : 0.f);
          const float acc = -fabsf(P[2] * dv) * sgn;
          xdd[i] = (fabsf(qdl[i]) < cutoff) ? 0.f : acc;
          const float ratio = fminf(dv, P[1] - 1e-6f) / P[1];
          dg[i] = P[3] / (1.0f - ratio * ratio);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
          if (i >= n_dof) continue;
          float fi = 0.f;
#pragma unroll
          for (int j = 0; j < N; ++j) {
            if (j >= n_dof) continue;
            const float a = (i == j) ? dg[i] : P[3] / 1.0f;
            A[i][j] += (double)a;
            fi += a * xdd[j];
          }
          fv[i] += (double)fi;
        }
      } else if (lf.kind == RMP2_LEAF_JOINT_LIMIT_AVOIDANCE || lf.kind == RMP2_LEAF_TARGET_POLICY) {
        // dense metrics built from a stretched direction zeta:  A_ij = cw_j * (beta zeta_i zeta_j + (1-beta) d_ij) * w
        float cw[N], zeta[N], beta, wsc;
        if (lf.kind == RMP2_LEAF_JOINT_LIMIT_AVOIDANCE) {
          // rmp.py:357-382; A = w * H broadcasts over the LAST axis: column scaling (quirk Q2)
          const float rr = 0.15f;
          const float c2 = (float)(-3.0 / (0.15 * 0.15)), c3 = (float)(2.0 / (0.15 * 0.15 * 0.15));
          const float qd_max = (float)(20.0 * (2.0 * 3.14159265358979323846) / 60.0);
          float v[N], s2 = 0.f;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const float range = lf.vb[i] - lf.va[i];
            const float du = (lf.vb[i] - ql[i]) / range;
            const float dl = (ql[i] - lf.va[i]) / range;
            const float d = fminf(du, dl);
            const float spline = c3 * (d * d * d) + c2 * (d * d) + 0.f * d + 1.0f;
            cw[i] = (i < n_dof) ? (d > rr ? 0.f : spline) : 0.f;
            v[i] = qdl[i] / qd_max;
            s2 += v[i] * v[i];
            xdd[i] = -P[0] * ql[i] - P[1] * qdl[i];
          }
          const float nrm = sqrtf(s2);
          const float hh = nrm + 1.0f / 5.0f * logf(1.0f + expf(-2.0f * 5.0f * nrm));
#pragma unroll
          for (int i = 0; i < N; ++i) zeta[i] = v[i] / hh;
          beta = 0.9f;
          wsc = 1.0f;
        } else {
          // rmp.py:241-260 on the identity map (goal is an n-vector)
          const float alpha = P[0], beta_d = P[1], c = P[2];
          float v[N], s2 = 0.f;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            v[i] = (i < n_dof) ? my_goal[lf.goal_offset + i] - ql[i] : 0.f;
            s2 += v[i] * v[i];
          }
          const float vn = sqrtf(s2);
          const float hq = vn + c * logf(1.0f + expf(-2.0f * c * vn));
          const float inv_h = 1.0f / hq;
          float f2 = 0.f;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            xdd[i] = alpha * (inv_h * v[i]) - beta_d * qdl[i];
            f2 += xdd[i] * xdd[i];
            cw[i] = 1.0f;
          }
          const float fn = sqrtf(f2);
          const float hs = fn + 1.0f / c * logf(1.0f + expf(-2.0f * c * fn));
#pragma unroll
          for (int i = 0; i < N; ++i) zeta[i] = xdd[i] / hs;
          beta = 1.0f - expf(-0.5f * (vn * vn) / 1.0f);
          wsc = expf(-vn / 3.0f);
        }
        const float omb = 1.0f - beta;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          if (i >= n_dof) continue;
          float fi = 0.f;
#pragma unroll
          for (int j = 0; j < N; ++j) {
            if (j >= n_dof) continue;
            const float Hij = beta * (zeta[i] * zeta[j]) + omb * (i == j ? 1.f : 0.f);
            const float a = (lf.kind == RMP2_LEAF_JOINT_LIMIT_AVOIDANCE) ? cw[j] * Hij : wsc * Hij;
            A[i][j] += (double)a;
            fi += a * xdd[j];
          }
          fv[i] += (double)fi;
        }
      }
    }

    // a dof whose state is not finite makes the robot's system non-finite by construction (rmp2_quad.h, same place): the
    // resolve answers NaN with RMP2_STATUS_NONFINITE also where no leaf carried the value into the system (an Inf velocity
    // behind out-of-range pairs only)
#pragma unroll
    for (int i = 0; i < N; ++i)
      fv[i] = (fabsf(ql[i]) < 3.0e38f && fabsf(qdl[i]) < 3.0e38f) ? fv[i] : (double)__builtin_nanf("");
#undef ql
#undef qdl
    // optional debug outputs: the combined metric / force before the resolve
    if (pass == (STRICT ? 1 : 0) && live) {
      if (out.M) {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
          for (int j = 0; j < N; ++j)
            if (i < n_dof && j < n_dof) out.M[((size_t)robot * n_dof + i) * n_dof + j] = A[i][j];
      }
      if (out.f) {
#pragma unroll
        for (int i = 0; i < N; ++i)
          if (i < n_dof) out.f[(size_t)robot * n_dof + i] = fv[i];
      }
    }
    // padding dofs of the template: identity rows so that they resolve to qdd = 0
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i >= n_dof) A[i][i] = 1.0;

    // ---- resolve   rmp.py:153-154 -----------------------------------------------------
    // The result goes straight to the LDS output tile so that no fp64 result registers stay
    // live across a second pass.
    if (STRICT) {
      double x[N];
      // a metric / force with NaN or Inf resolves to NaN (tf.linalg.pinv of such a matrix, rmp.py:153): the Jacobi iteration
      // would skip the NaN rows and return the pseudo-inverse of what is left
      bool finite_in = true;
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) finite_in = finite_in && (fabs(A[i][j]) < 1.7e308);
        finite_in = finite_in && (fabs(fv[i]) < 1.7e308);
      }
      int dropped = 0;
      if (finite_in) {
        dropped = pinv_solve<N>(A, fv, n_dof, x);
      } else {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = __builtin_nan("");
      }
      if (dropped) status |= RMP2_STATUS_RANK_DROP;
      bool finite = true;
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (i < n_dof) {
          finite = finite && (fabs(x[i]) < 1.7e308);
          my_out[i] = (float)x[i];
        }
      if (!finite) status |= RMP2_STATUS_NONFINITE;
    } else if (pass == 0) {
      double x[N];
      singular = lu_solve<N>(A, fv, x);
      bool finite = true;
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (i < n_dof) {
          finite = finite && (fabs(x[i]) < 1.7e308);
          my_out[i] = (float)x[i];
        }
      singular = singular || !finite;  // let the careful path have a look before reporting NaN/Inf
      if (!__any(singular && live)) break;
    } else if (singular) {
      double W[N * (N + 1)], T[N * (N + 1)], xp[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) W[i * (N + 1) + j] = A[i][j];
        W[i * (N + 1) + N] = fv[i];
      }
      status |= RMP2_STATUS_PINV_PATH;
      bool finite_in = true;  // a metric / force with NaN or Inf resolves to NaN (as the reference's pinv does):
      for (int i = 0; i < N * (N + 1); ++i) finite_in = finite_in && (fabs(W[i]) < 1.7e308);  // no point iterating on it
      if (!finite_in) {
        for (int i = 0; i < N; ++i) xp[i] = __builtin_nan("");
      } else if (!lu_pivot_compact(W, T, N, xp)) {
        const int dropped = pinv_solve_compact(W, N, n_dof, xp);
        if (dropped) status |= RMP2_STATUS_RANK_DROP;
      }
      bool finite = true;
      for (int i = 0; i < n_dof; ++i) {
        finite = finite && (fabs(xp[i]) < 1.7e308);
        my_out[i] = (float)xp[i];
      }
      if (!finite) status |= RMP2_STATUS_NONFINITE;
    }
  }

  // ---- coalesced store of the qdd tile ----------------------------------------------------
  __syncthreads();
  {
    const float* tile = &lds[Lds<N>::kOut];
    const int count = min(kWave, R - r0) * n_dof;
    float* go = out.qdd + (size_t)r0 * n_dof;
    for (int i = lane; i < count; i += kWave) go[i] = tile[i];
  }
  if (out.status && live) out.status[robot] = status;
}

// The resolve on its own: q'' = pinv(M) f for every robot (rmp.py:153-154, TensorFlow's cutoff), a lane per robot, register-resident
// one-sided Jacobi (rmp2_solve.h pinv_solve).  Second kernel of the strict / rank-deficient control step at fleet size: the quad
// mapping (culled, split pair loops) stops behind the combined metric and force, this kernel resolves them -- the lane-per-robot
// step kernel that carries the same resolve walks all 256 pairs of a robot in one lane (285 us per step for config 3 at 65 536
// robots).
template <int N>
__global__ void __launch_bounds__(kWave)
rmp2_pinv_kernel(const double* __restrict__ M, const double* __restrict__ f, float* __restrict__ qdd, uint32_t* __restrict__ status_out,
                 int n_dof, int R) {
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  // M [n_dof * n_dof][R], f [n_dof][R]: robot index fastest (the quad kernel's skip_resolve layout) -- coalesced here
  double A[N][N], fv[N], x[N];
  bool finite_in = true;
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      A[i][j] = (i < n_dof && j < n_dof) ? M[(size_t)(i * n_dof + j) * R + robot] : (i == j ? 1.0 : 0.0);  // padding dofs: identity
      finite_in = finite_in && (fabs(A[i][j]) < 1.7e308);                                                  // rows, q'' = 0
    }
    fv[i] = i < n_dof ? f[(size_t)i * R + robot] : 0.0;
    finite_in = finite_in && (fabs(fv[i]) < 1.7e308);
  }
  uint32_t status = 0u;
  if (finite_in) {
    if (pinv_solve<N>(A, fv, n_dof, x)) status |= RMP2_STATUS_RANK_DROP;
  } else {  // (as the reference's pinv of a matrix with NaN / Inf)
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = __builtin_nan("");
  }
  bool finite = true;
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (i < n_dof) {
      finite = finite && (fabs(x[i]) < 1.7e308);
      qdd[(size_t)robot * n_dof + i] = (float)x[i];
    }
  if (!finite) status |= RMP2_STATUS_NONFINITE;
  if (status_out) status_out[robot] = status;
}

// Debug outputs of the two-kernel strict step: the combined systems sit robot-index-FASTEST in the handle's buffer (what the
// two kernels exchange); the caller's M [R][n][n] and f [R][n] are robot-index-slowest.
__global__ void __launch_bounds__(kWave)
rmp2_system_copy_kernel(const double* __restrict__ Ms, const double* __restrict__ fs, double* __restrict__ M, double* __restrict__ f,
                        int n, int R) {
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  for (int e = 0; e < n * n; ++e)
    if (M) M[(size_t)robot * n * n + e] = Ms[(size_t)e * R + robot];
  for (int i = 0; i < n; ++i)
    if (f) f[(size_t)robot * n + i] = fs[(size_t)i * R + robot];
}

// =========================================================================================
// device: one leaf on its own -- the reference's leaf protocol  rmp.evaluate(x, xd) -> (xdd, A)
// (rmp2.py:25-29, rmp.py:202-206), one lane per row of the batch, libm-accurate formulas
// =========================================================================================
__global__ void __launch_bounds__(kWave)
rmp2_leaf_kernel(rmp2_leaf lf, int k, const float* __restrict__ x, const float* __restrict__ xd,
                 const float* __restrict__ goal, const float* __restrict__ dist, const float* __restrict__ nvec,
                 float* __restrict__ xdd_o, float* __restrict__ A_o, int B) {
  const int b = blockIdx.x * kWave + threadIdx.x;
  if (b >= B) return;
  const float* P = lf.params;
  const float* xb = x + (size_t)b * k;
  const float* vb = xd + (size_t)b * k;
  float* xo = xdd_o + (size_t)b * k;
  float* Ao = A_o + (size_t)b * k * k;
  for (int i = 0; i < k * k; ++i) Ao[i] = 0.f;
  auto put_sym3 = [&](const float S[6]) {
    Ao[0] = S[0], Ao[1] = S[1], Ao[2] = S[2];
    Ao[3] = S[1], Ao[4] = S[3], Ao[5] = S[4];
    Ao[6] = S[2], Ao[7] = S[4], Ao[8] = S[5];
  };
  switch (lf.kind) {
    case RMP2_LEAF_TARGET_ATTRACTOR: {  // rmp2.py:52-83, k = 3
      const float xx[3] = {xb[0], xb[1], xb[2]}, vv[3] = {vb[0], vb[1], vb[2]}, g[3] = {goal[0], goal[1], goal[2]};
      float acc[3], S[6];
      leaf_target_attractor(P, xx, vv, g, acc, S);
      for (int i = 0; i < 3; ++i) xo[i] = acc[i];
      put_sym3(S);
    } break;
    case RMP2_LEAF_OBSTACLE_AVOIDANCE: {  // rmp2.py:183-196, k = 1
      float acc, met;
      leaf_obstacle_avoidance(P, xb[0], vb[0], acc, met);
      xo[0] = acc;
      Ao[0] = met;
    } break;
    case RMP2_LEAF_COLLISION_AVOIDANCE: {  // rmp.py:264-315, k = 3, data-fed d and n
      const float nv[3] = {nvec[3 * b], nvec[3 * b + 1], nvec[3 * b + 2]}, vv[3] = {vb[0], vb[1], vb[2]};
      float acc[3], w;
      leaf_collision_avoidance(P, dist[b], nv, vv, acc, w);
      for (int i = 0; i < 3; ++i) xo[i] = acc[i], Ao[4 * i] = w;
    } break;
    case RMP2_LEAF_JOINT_DAMPING: {  // rmp2.py:127-137
      float s2 = 0.f;
      for (int i = 0; i < k; ++i) s2 += vb[i] * vb[i];
      const float nrm = sqrtf(s2), m = P[1] * nrm + P[2];
      for (int i = 0; i < k; ++i) xo[i] = -(P[0] * nrm) * vb[i], Ao[i * k + i] = m;
    } break;
    case RMP2_LEAF_CSPACE_BIASING: {  // rmp2.py:212-226
      float s2 = 0.f;
      for (int i = 0; i < k; ++i) s2 += (xb[i] - lf.vec_a[i]) * (xb[i] - lf.vec_a[i]);
      const float en = sqrtf(s2), m = P[0] + P[4];
      for (int i = 0; i < k; ++i) {
        const float e = xb[i] - lf.vec_a[i];
        const float pos = (en < P[3]) ? (-e * P[1]) : (-P[3] * (e / en) * P[1]);
        xo[i] = pos + (-P[2] * vb[i]);
        Ao[i * k + i] = m;
      }
    } break;
    case RMP2_LEAF_CONFIG_SPACE_BIASING: {  // rmp.py:330-347
      for (int i = 0; i < k; ++i) xo[i] = P[0] * (lf.vec_a[i] - xb[i]) - P[1] * vb[i], Ao[i * k + i] = P[2];
    } break;
    case RMP2_LEAF_JOINT_VELOCITY_CAP: {  // rmp2.py:100-112, metric on the FULL matrix (quirk Q4)
      const float cutoff = P[0] - P[1];
      for (int i = 0; i < k; ++i) {
        const float dv = fabsf(vb[i]) - cutoff;
        const float sgn = (vb[i] > 0.f) ? 1.f : (vb[i] < 0.f ? -1.f : 0.f);
        xo[i] = (fabsf(vb[i]) < cutoff) ? 0.f : -fabsf(P[2] * dv) * sgn;
        const float ratio = fminf(dv, P[1] - 1e-6f) / P[1];
        for (int j = 0; j < k; ++j) Ao[i * k + j] = (i == j) ? P[3] / (1.0f - ratio * ratio) : P[3] / 1.0f;
      }
    } break;
    case RMP2_LEAF_JOINT_LIMIT_AVOIDANCE: {  // rmp.py:357-382, A = H diag(w) (quirk Q2)
      const float rr = 0.15f, c2 = (float)(-3.0 / (0.15 * 0.15)), c3 = (float)(2.0 / (0.15 * 0.15 * 0.15));
      const float qd_max = (float)(20.0 * (2.0 * 3.14159265358979323846) / 60.0);
      float cw[RMP2_MAX_DOF], zeta[RMP2_MAX_DOF], s2 = 0.f;
      for (int i = 0; i < k; ++i) {
        const float range = lf.vec_b[i] - lf.vec_a[i];
        const float d = fminf((lf.vec_b[i] - xb[i]) / range, (xb[i] - lf.vec_a[i]) / range);
        cw[i] = d > rr ? 0.f : c3 * (d * d * d) + c2 * (d * d) + 0.f * d + 1.0f;
        zeta[i] = vb[i] / qd_max;
        s2 += zeta[i] * zeta[i];
        xo[i] = -P[0] * xb[i] - P[1] * vb[i];
      }
      const float nrm = sqrtf(s2), hh = nrm + 1.0f / 5.0f * logf(1.0f + expf(-2.0f * 5.0f * nrm));
      for (int i = 0; i < k; ++i) zeta[i] /= hh;
      for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) Ao[i * k + j] = cw[j] * (0.9f * (zeta[i] * zeta[j]) + 0.1f * (i == j ? 1.f : 0.f));
    } break;
    case RMP2_LEAF_TARGET_POLICY: {  // rmp.py:241-260 on a k-dimensional task space (one row = one evaluation: the
      const float alpha = P[0], beta_d = P[1], c = P[2];  // reference's norms are global, i.e. B = 1)
      float v[RMP2_MAX_DOF], s2 = 0.f, f2 = 0.f;
      for (int i = 0; i < k; ++i) v[i] = goal[i] - xb[i], s2 += v[i] * v[i];
      const float vn = sqrtf(s2);
      const float inv_h = 1.0f / (vn + c * logf(1.0f + expf(-2.0f * c * vn)));
      for (int i = 0; i < k; ++i) xo[i] = alpha * (inv_h * v[i]) - beta_d * vb[i], f2 += xo[i] * xo[i];
      const float fn = sqrtf(f2), hs = fn + 1.0f / c * logf(1.0f + expf(-2.0f * c * fn));
      const float beta = 1.0f - expf(-0.5f * (vn * vn) / 1.0f), w = expf(-vn / 3.0f);
      for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j)
          Ao[i * k + j] = w * (beta * ((xo[i] / hs) * (xo[j] / hs)) + (1.0f - beta) * (i == j ? 1.f : 0.f));
    } break;
    default: break;
  }
}

// =========================================================================================
// host: handle, program compiler, launches
// =========================================================================================
thread_local std::string g_create_error;
std::mutex g_fence_mutex;                   // guards g_attached_fences
std::map<void*, int> g_attached_fences;     // fence -> number of handles it is attached to (rmp2_set_step_fence)

}  // namespace


namespace {

int fail(rmp2_handle* h, int code, const std::string& msg) {
  if (h)
    h->error = msg;
  else
    g_create_error = msg;
  return code;
}

#define HIP_TRY(h, expr)                                                                       \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(h, RMP2_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));         \
  } while (0)

// Every launching entry point makes the handle's device the calling thread's current device first (include/rmp2.h,
// "Rules of the boundary"): a process that drives two engines on two devices must not launch on whichever device the
// last rmp2_create left current.
int use_device(rmp2_handle* h) {
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != h->device) HIP_TRY(h, hipSetDevice(h->device));
  return RMP2_OK;
}

// True while `s` is being captured into a graph: no allocation, no synchronisation.
bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  return s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

// A grow-on-demand buffer of the handle: the old allocation freed (hipFree synchronises the device: no launch still reads it),
// `bytes` allocated in its place.
template <class T>
int realloc_device(rmp2_handle* h, T** p, size_t bytes) {
  if (*p) HIP_TRY(h, hipFree(*p));
  *p = nullptr;
  HIP_TRY(h, hipMalloc(p, bytes));
  return RMP2_OK;
}

// Structural zeros of the position Jacobian.  The reference differentiates the frame's position through the chain of LOCAL
// transforms (kinematics.py:243-270): where the origin of frame f lies ON the axis of a revolute ancestor joint j for every q
// -- joint f's own axis; consecutive joints whose <origin xyz> is 0 (Panda joints 1/2, 5/6); a tool frame straight up the last
// joint's axis -- its column d p_f / d q_j is EXACTLY zero there.  The kernels form columns in world coordinates,
// z_j x (p_f - o_j), where such a lever comes out as fp32 rounding noise (1e-8): harmless beside any other metric on dof j, but
// in a set that gives dof j nothing else (the reference's Panda experiments 01-03 carry only a target policy) the noise column
// is a "real" tiny one, sigma ~ 1e-16 sigma_max is kept by the pseudo-inverse's cutoff now and then, and q-double-dot_j =
// (noise) / (noise^2) ~ 1e7 where the reference returns 0 (found by tools/fuzz_parity.py).  So the compiler marks these
// (frame, dof) pairs -- bit 16 + j of DevOp::anc_mask -- and the kernels take the frame's own origin as the point of joint j's
// axis there: the lever of the origin is then exactly 0, and an attached point's lever is its offset from the origin.
// Decided in fp64 from the descriptor's constants at four random configurations; zero_of[f] bit j: structural.
static void structural_lever_zeros(const rmp2_robot& rb, std::vector<uint32_t>& zero_of) {
  const int F0 = rb.n_frames, n = rb.n_dof;
  zero_of.assign(F0, 0u);
  std::vector<uint32_t> cand(F0, 0u);
  for (int f = 0; f < F0; ++f)
    for (int j = f; j >= 0; j = rb.parent[j])
      if (rb.joint_type[j] == RMP2_JOINT_REVOLUTE && rb.q_index[j] >= 0) cand[f] |= 1u << rb.q_index[j];
  uint64_t lcg = 0x9E3779B97F4A7C15ull;
  auto uniform = [&]() {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(lcg >> 11) / 9007199254740992.0;
  };
  struct Pose {
    double R[9], p[3];
  };
  std::vector<Pose> T(F0);
  for (int trial = 0; trial < 4; ++trial) {
    double q[RMP2_MAX_DOF];
    for (int j = 0; j < n; ++j) q[j] = 6.0 * uniform() - 3.0;
    for (int f = 0; f < F0; ++f) {
      Pose A;  // T_parent @ T_const
      const float* C = rb.T_const[f];
      if (rb.parent[f] < 0) {
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c) A.R[3 * r + c] = C[4 * r + c];
          A.p[r] = C[4 * r + 3];
        }
      } else {
        const Pose& Pp = T[rb.parent[f]];
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c)
            A.R[3 * r + c] = Pp.R[3 * r] * C[c] + Pp.R[3 * r + 1] * C[4 + c] + Pp.R[3 * r + 2] * C[8 + c];
          A.p[r] = Pp.R[3 * r] * C[3] + Pp.R[3 * r + 1] * C[7] + Pp.R[3 * r + 2] * C[11] + Pp.p[r];
        }
      }
      const double qv = (rb.joint_type[f] != RMP2_JOINT_FIXED && rb.q_index[f] >= 0) ? q[rb.q_index[f]] : 0.0;
      const double u[3] = {rb.axis[f][0], rb.axis[f][1], rb.axis[f][2]};
      if (rb.joint_type[f] == RMP2_JOINT_REVOLUTE) {  // Rodrigues (kinematics.py:103-121)
        const double c = std::cos(qv), s = std::sin(qv);
        const double K[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
        double Rv[9];
        for (int r = 0; r < 3; ++r)
          for (int cc = 0; cc < 3; ++cc) Rv[3 * r + cc] = (r == cc ? c : 0.0) + (1.0 - c) * u[r] * u[cc] + s * K[3 * r + cc];
        double Rn[9];
        for (int r = 0; r < 3; ++r)
          for (int cc = 0; cc < 3; ++cc) Rn[3 * r + cc] = A.R[3 * r] * Rv[cc] + A.R[3 * r + 1] * Rv[3 + cc] + A.R[3 * r + 2] * Rv[6 + cc];
        std::memcpy(A.R, Rn, sizeof(Rn));
      } else if (rb.joint_type[f] == RMP2_JOINT_PRISMATIC) {
        for (int r = 0; r < 3; ++r) A.p[r] += (A.R[3 * r] * u[0] + A.R[3 * r + 1] * u[1] + A.R[3 * r + 2] * u[2]) * qv;
      }
      T[f] = A;
    }
    for (int f = 0; f < F0; ++f)
      for (int j = f; j >= 0; j = rb.parent[j]) {
        if (rb.joint_type[j] != RMP2_JOINT_REVOLUTE || rb.q_index[j] < 0) continue;
        const Pose& J = T[j];
        const double z[3] = {J.R[0] * rb.axis[j][0] + J.R[1] * rb.axis[j][1] + J.R[2] * rb.axis[j][2],
                             J.R[3] * rb.axis[j][0] + J.R[4] * rb.axis[j][1] + J.R[5] * rb.axis[j][2],
                             J.R[6] * rb.axis[j][0] + J.R[7] * rb.axis[j][1] + J.R[8] * rb.axis[j][2]};
        const double l[3] = {T[f].p[0] - J.p[0], T[f].p[1] - J.p[1], T[f].p[2] - J.p[2]};
        const double c[3] = {z[1] * l[2] - z[2] * l[1], z[2] * l[0] - z[0] * l[2], z[0] * l[1] - z[1] * l[0]};
        const double cn = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), ln = std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
        if (cn > 1e-11 * (1.0 + ln)) cand[f] &= ~(1u << rb.q_index[j]);
      }
  }
  zero_of = cand;
}

// Compile the descriptor into the device program: depth-first schedule with save/restore slots
// (same algorithm as urdf.py:depth_first_schedule).
// prune = true (control-step kernels): frames that are not an ancestor-or-self of a frame carrying a
// leaf are dropped (they cannot influence qdd), and FIXED frames without a leaf are folded into their
// children's constant transform (T_c' = T_fixed @ T_c, formed in fp64; exact up to one fp32 rounding
// of the folded constant).  prune = false: every frame is visited (forward-kinematics entry points).
int compile_program(const rmp2_desc& d, DevProgram& P, int& n_slots, std::string& err, bool prune,
                    std::vector<HexOp>* hops = nullptr) {
  const rmp2_robot& rb = d.robot;
  const int F0 = rb.n_frames, n = rb.n_dof;
  if (F0 < 0 || F0 > RMP2_MAX_FRAMES) return err = "n_frames out of range", RMP2_ERR_INVALID_ARGUMENT;
  if (n < 1 || n > RMP2_MAX_DOF) return err = "n_dof out of range", RMP2_ERR_INVALID_ARGUMENT;
  if (d.n_leaves < 0 || d.n_leaves > RMP2_MAX_LEAVES) return err = "n_leaves out of range", RMP2_ERR_INVALID_ARGUMENT;
  std::memset(&P, 0, sizeof(P));
  for (int i = 0; i < F0; ++i) {
    const int p = rb.parent[i];
    if (p >= i || p < -1) return err = "parent[] must be topologically ordered (parent < child)", RMP2_ERR_INVALID_ARGUMENT;
    if (rb.joint_type[i] < 0 || rb.joint_type[i] > 2) return err = "bad joint_type", RMP2_ERR_INVALID_ARGUMENT;
    if (rb.q_index[i] >= n || rb.q_index[i] < -1)  // (-1: a joint held at q = 0; found by the sanitizer run: -2 used to pass)
      return err = "q_index out of range (-1 = evaluated at q = 0, else 0 .. n_dof - 1)", RMP2_ERR_INVALID_ARGUMENT;
  }
  // working tree (possibly pruned / folded); wf[i] refers to original frame wf[i].orig
  struct WFrame {
    int orig, parent;
    double Tc[12];
  };
  std::vector<WFrame> wf;
  {
    std::vector<char> has_leaf(F0, 0), needed(F0, prune ? 0 : 1), keep(F0, 0);
    for (int l = 0; l < d.n_leaves; ++l)
      if (d.leaves[l].taskmap != RMP2_TASKMAP_IDENTITY && d.leaves[l].frame >= 0 && d.leaves[l].frame < F0)
        has_leaf[d.leaves[l].frame] = 1;
    for (int f = F0 - 1; f >= 0; --f)
      if (has_leaf[f])
        for (int j = f; j >= 0 && !needed[j]; j = rb.parent[j]) needed[j] = 1;
    std::vector<int> new_index(F0, -1);
    for (int f = 0; f < F0; ++f) {
      keep[f] = needed[f] && !(prune && rb.joint_type[f] == RMP2_JOINT_FIXED && !has_leaf[f]);
      if (!keep[f]) continue;
      WFrame w;
      w.orig = f;
      for (int c = 0; c < 12; ++c) w.Tc[c] = rb.T_const[f][c];
      int p = rb.parent[f];
      while (p >= 0 && !keep[p]) {  // fold the dropped (fixed, leaf-less) ancestors: T = T_p @ T
        double T[12];
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c)
            T[4 * r + c] = (double)rb.T_const[p][4 * r] * w.Tc[c] + (double)rb.T_const[p][4 * r + 1] * w.Tc[4 + c] +
                           (double)rb.T_const[p][4 * r + 2] * w.Tc[8 + c];
          T[4 * r + 3] = (double)rb.T_const[p][4 * r] * w.Tc[3] + (double)rb.T_const[p][4 * r + 1] * w.Tc[7] +
                         (double)rb.T_const[p][4 * r + 2] * w.Tc[11] + (double)rb.T_const[p][4 * r + 3];
        }
        std::memcpy(w.Tc, T, sizeof(T));
        p = rb.parent[p];
      }
      w.parent = p < 0 ? -1 : new_index[p];
      new_index[f] = (int)wf.size();
      wf.push_back(w);
    }
  }
  const int F = (int)wf.size();
  std::vector<std::vector<int>> children(F);
  std::vector<int> roots;
  for (int i = 0; i < F; ++i) (wf[i].parent < 0 ? roots : children[wf[i].parent]).push_back(i);
  std::vector<int> order, stack(roots.rbegin(), roots.rend());
  while (!stack.empty()) {
    const int i = stack.back();
    stack.pop_back();
    order.push_back(i);
    for (auto it = children[i].rbegin(); it != children[i].rend(); ++it) stack.push_back(*it);
  }
  std::vector<int> pos(F), slot_of(F, -1), free_at;
  for (int k = 0; k < F; ++k) pos[order[k]] = k;
  uint32_t rev_mask = 0;
  std::vector<int> dof_owner(n, -1);
  for (int f0 = 0; f0 < F0; ++f0) {  // dof ownership / revolute mask over ALL frames of the robot
    const int qi = (rb.joint_type[f0] == RMP2_JOINT_FIXED) ? -1 : rb.q_index[f0];
    if (qi < 0) continue;
    if (dof_owner[qi] >= 0) return err = "two joints share one q index", RMP2_ERR_INVALID_ARGUMENT;
    dof_owner[qi] = f0;
    if (rb.joint_type[f0] == RMP2_JOINT_REVOLUTE) rev_mask |= 1u << qi;
  }
  std::vector<uint32_t> lever_zero;
  structural_lever_zeros(rb, lever_zero);
  for (int k = 0; k < F; ++k) {
    const int w = order[k], p = wf[w].parent, f = wf[w].orig;
    DevOp& op = P.ops[k];
    op.frame = f;
    op.restore = (p < 0) ? -2 : ((k > 0 && order[k - 1] == p) ? -1 : slot_of[p]);
    op.save = -1;
    int last_use = -1;
    for (int c : children[w])
      if (pos[c] != k + 1) last_use = std::max(last_use, pos[c]);
    if (last_use >= 0) {
      int s = -1;
      for (size_t t = 0; t < free_at.size(); ++t)
        if (free_at[t] < k) {
          s = (int)t;
          break;
        }
      if (s < 0) {
        free_at.push_back(0);
        s = (int)free_at.size() - 1;
      }
      free_at[s] = last_use;
      slot_of[w] = s;
      op.save = s;
    }
    op.jtype = rb.joint_type[f];
    op.qidx = (op.jtype == RMP2_JOINT_FIXED) ? -1 : rb.q_index[f];
    uint32_t mask = 0;
    for (int j = f; j >= 0; j = rb.parent[j])
      if (rb.joint_type[j] != RMP2_JOINT_FIXED && rb.q_index[j] >= 0) mask |= 1u << rb.q_index[j];
    op.anc_mask = mask | ((lever_zero[f] & mask & 0xffffu) << 16);  // (bits 16 + j: structural_lever_zeros above)
    for (int c = 0; c < 3; ++c) op.axis[c] = rb.axis[f][c];
    for (int c = 0; c < 12; ++c) op.Tc[c] = (float)wf[w].Tc[c];
  }
  {  // tables of the 16-lane kernel: pointer-jumping ancestors, per-dof joint op and strict ancestor dofs
    std::vector<int> parent_op(F, -1), depth(F, 1);
    int deepest = F > 0 ? 1 : 0;
    for (int k = 0; k < F; ++k) {
      const int p = wf[order[k]].parent;
      parent_op[k] = p < 0 ? -1 : pos[p];
      depth[k] = p < 0 ? 1 : depth[pos[p]] + 1;  // depth-first order: the parent's op precedes k
      deepest = std::max(deepest, depth[k]);
    }
    int L = 0;
    while ((1 << L) < deepest) ++L;
    P.hex.n_levels = L;
    P.hex.is_chain = 1;
    for (int k = 0; k < F; ++k)
      if (parent_op[k] != k - 1) P.hex.is_chain = 0;
    for (int l = 0; l < 5; ++l)
      for (int k = 0; k < kMaxOps; ++k) P.hex.jump[l][k] = -1;
    for (int k = 0; k < F; ++k) P.hex.jump[0][k] = parent_op[k];
    for (int l = 1; l < 5; ++l)
      for (int k = 0; k < F; ++k) {
        const int j = P.hex.jump[l - 1][k];
        P.hex.jump[l][k] = j < 0 ? -1 : P.hex.jump[l - 1][j];
      }
    for (int k = 0; k < kMaxOps; ++k) P.hex.op_anc[k] = 0u;
    for (int k = 0; k < F; ++k) P.hex.op_anc[k] = (1u << k) | (parent_op[k] >= 0 ? P.hex.op_anc[parent_op[k]] : 0u);
    if (hops) {
      hops->assign(F, HexOp{});
      for (int k = 0; k < F; ++k) {
        const int w = order[k], f = wf[w].orig;
        const double* Tc = wf[w].Tc;
        const double u[3] = {rb.axis[f][0], rb.axis[f][1], rb.axis[f][2]};
        const bool rev = rb.joint_type[f] == RMP2_JOINT_REVOLUTE, pri = rb.joint_type[f] == RMP2_JOINT_PRISMATIC;
        const double ux[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
        HexOp& ho = (*hops)[k];
        for (int r = 0; r < 3; ++r) {
          const double Rc[3] = {Tc[4 * r], Tc[4 * r + 1], Tc[4 * r + 2]};
          const double Ru = Rc[0] * u[0] + Rc[1] * u[1] + Rc[2] * u[2];
          for (int c = 0; c < 3; ++c) {
            const double a0 = Ru * u[c];                                              // (Rc u u^T)_rc
            const double a2 = Rc[0] * ux[c] + Rc[1] * ux[3 + c] + Rc[2] * ux[6 + c];  // (Rc [u]x)_rc
            ho.A0[3 * r + c] = (float)(rev ? a0 : Rc[c]);
            ho.A1[3 * r + c] = (float)(rev ? Rc[c] - a0 : 0.0);
            ho.A2[3 * r + c] = (float)(rev ? a2 : 0.0);
          }
          ho.tc[r] = (float)Tc[4 * r + 3];
          ho.tu[r] = (float)(pri ? Ru : 0.0);
        }
      }
    }
  }
  n_slots = (int)free_at.size();
  P.n_ops = F;
  P.n_dof = n;
  P.n_frames = F0;
  P.n_leaves = d.n_leaves;
  P.goal_floats = d.goal_floats;
  P.solve_mode = d.solve_mode;
  P.rev_mask = rev_mask;
  if (d.solve_mode != RMP2_SOLVE_AUTO && d.solve_mode != RMP2_SOLVE_PINV)
    return err = "unknown solve_mode", RMP2_ERR_INVALID_ARGUMENT;

  // leaves: validate, copy, bucket by task map
  int nfk = 0, nid = 0, n_dist = 0;
  for (int l = 0; l < d.n_leaves; ++l) {
    const rmp2_leaf& s = d.leaves[l];
    DevLeaf& t = P.leaves[l];
    t.kind = s.kind;
    t.taskmap = s.taskmap;
    t.frame = s.frame;
    t.goal_offset = s.goal_offset;
    t.index = l;
    // (row of rmp2_obstacles.link_capsules: the leaves that consume per-pair obstacle data, in descriptor order)
    t.dist_ordinal = (s.taskmap == RMP2_TASKMAP_FK_DISTANCE || s.taskmap == RMP2_TASKMAP_FK_POINT) ? n_dist++ : -1;
    std::memcpy(t.P, s.params, sizeof(t.P));
    std::memcpy(t.va, s.vec_a, sizeof(t.va));
    std::memcpy(t.vb, s.vec_b, sizeof(t.vb));
    if (s.kind == RMP2_LEAF_OBSTACLE_AVOIDANCE) {
      // reciprocals of the length scales (two of them pre-multiplied by log2 e), formed in double
      // (used by the quad kernel's pair loop)
      const double estd = s.params[9], rstd = s.params[6], dstd = s.params[2], glen = s.params[4], rad = s.params[7];
      t.vb[0] = (float)(1.0 / estd);
      t.vb[1] = (float)(1.4426950408889634 / rstd);  // log2(e) / rstd
      t.vb[2] = (float)(1.0 / dstd);
      t.vb[3] = (float)(1.4426950408889634 / glen);  // log2(e) / gate_len
      t.vb[4] = (float)(1.0 / (rad * rad));
      t.vb[5] = (float)(2.0 / rad);
    }
    int goal_len = 0;
    bool ok = false;
    switch (s.taskmap) {
      case RMP2_TASKMAP_IDENTITY:
        ok = s.kind == RMP2_LEAF_JOINT_VELOCITY_CAP || s.kind == RMP2_LEAF_JOINT_DAMPING ||
             s.kind == RMP2_LEAF_CSPACE_BIASING || s.kind == RMP2_LEAF_JOINT_LIMIT_AVOIDANCE ||
             s.kind == RMP2_LEAF_CONFIG_SPACE_BIASING || s.kind == RMP2_LEAF_TARGET_POLICY;
        if (s.kind == RMP2_LEAF_TARGET_POLICY) goal_len = n;
        break;
      case RMP2_TASKMAP_FK_POSITION:
        ok = s.kind == RMP2_LEAF_TARGET_ATTRACTOR || s.kind == RMP2_LEAF_TARGET_POLICY;
        goal_len = 3;
        break;
      case RMP2_TASKMAP_FK_DISTANCE: ok = s.kind == RMP2_LEAF_OBSTACLE_AVOIDANCE; break;
      case RMP2_TASKMAP_FK_POINT: ok = s.kind == RMP2_LEAF_COLLISION_AVOIDANCE; break;
      default: break;
    }
    if (!ok) return err = "leaf " + std::to_string(l) + ": this (kind, taskmap) pair has no kernel", RMP2_ERR_UNSUPPORTED;
    if (s.taskmap != RMP2_TASKMAP_IDENTITY && (s.frame < 0 || s.frame >= F0))
      return err = "leaf " + std::to_string(l) + ": frame out of range", RMP2_ERR_INVALID_ARGUMENT;
    if (goal_len && (s.goal_offset < 0 || s.goal_offset + goal_len > d.goal_floats))
      return err = "leaf " + std::to_string(l) + ": goal_offset/goal_floats inconsistent", RMP2_ERR_INVALID_ARGUMENT;
    if (s.taskmap == RMP2_TASKMAP_IDENTITY) P.id_leaves[nid++] = l;
  }
  for (int k = 0; k < F; ++k) {
    DevOp& op = P.ops[k];
    op.leaf_begin = nfk;
    for (int l = 0; l < d.n_leaves; ++l)
      if (d.leaves[l].taskmap != RMP2_TASKMAP_IDENTITY && d.leaves[l].frame == op.frame) P.fk_leaves[nfk++] = l;
    op.leaf_count = nfk - op.leaf_begin;
  }
  P.n_fk_leaves = nfk;
  P.n_leaf_ops = 0;
  for (int k = 0; k < F; ++k)
    if (P.ops[k].leaf_count > 0) P.leaf_ops[P.n_leaf_ops++] = k;
  for (int t = 0; t < P.n_leaf_ops; ++t) {
    const DevOp& o = P.ops[P.leaf_ops[t]];
    P.leaf_frames[t] = {P.leaf_ops[t], o.anc_mask, o.leaf_begin, o.leaf_count};
  }
  for (int i = 0; i < d.n_leaves; ++i) P.leaves[i].next_pair_leaf = -1;
  for (int i = 0; i < nfk; ++i) P.exec_leaves[i] = P.leaves[P.fk_leaves[i]];
  for (int i = 0, last = -1; i < nfk; ++i)   // chain of the FK_DISTANCE leaves in execution order (explicit-pair prefetch)
    if (P.exec_leaves[i].taskmap == RMP2_TASKMAP_FK_DISTANCE) {
      if (last >= 0) P.exec_leaves[last].next_pair_leaf = P.exec_leaves[i].index;
      last = i;
    }
  for (int i = 0; i < nid; ++i) P.exec_leaves[nfk + i] = P.leaves[P.id_leaves[i]];  // (nfk + nid = n_leaves <= RMP2_MAX_LEAVES)
  // the structured identity-leaf records of the quad kernel (rmp2_device.h IdLeafRec): all of them or none
  P.id_structured = nid > 0 ? 1 : 0;
  for (int i = 0; i < nid; ++i)
    if (!id_leaf_structured(P.leaves[P.id_leaves[i]].kind)) P.id_structured = 0;
  std::memset(P.id_recs, 0, sizeof(P.id_recs));
  for (int i = 0; i < nid && P.id_structured; ++i) {
    const DevLeaf& lf = P.leaves[P.id_leaves[i]];
    IdLeafRec& r = P.id_recs[i];
    r.kind = lf.kind;
    // (volatile: the three values are rounded to float one operation at a time, as the kernel forms them)
    volatile float cutoff = lf.P[0] - lf.P[1], rlimit = lf.P[1] - 1e-6f, msum = lf.P[0] + lf.P[4];
    r.cutoff = cutoff, r.rlimit = rlimit, r.msum = msum;
    for (int c = 0; c < RMP2_MAX_PARAMS; ++c) r.P[c] = lf.P[c];
    for (int c = 0; c < RMP2_MAX_DOF; ++c) r.va[c] = lf.va[c];
  }
  for (int k = 0; k < F; ++k) {
    const DevOp& o = P.ops[k];
    P.ops[k].ctl = (o.restore + 2) | ((o.save + 1) << 2) | (o.jtype << 4) | ((o.qidx + 1) << 6) | ((o.leaf_count > 0 ? 1 : 0) << 11);
    // bits 12..17: row of rmp2_obstacles.link_capsules of the frame's FK_DISTANCE leaf + 1 (the lean link-geometry builds of the
    // quad mapping form the link's world segment in the walk); frames with two such leaves keep the attached-record builds
    // (rmp2_handle::link_rows_ok)
    int n_dist_here = 0;
    for (int i = 0; i < o.leaf_count; ++i) {
      const DevLeaf& lf = P.leaves[P.fk_leaves[o.leaf_begin + i]];
      if (lf.taskmap == RMP2_TASKMAP_FK_DISTANCE) {
        if (n_dist_here++ == 0) P.ops[k].ctl |= (lf.dist_ordinal + 1) << 12;
      }
    }
    (void)n_dist_here;
  }
  // the op that owns each dof (its frame's origin is the joint origin o_j, its world axis z_j): 5 bits per dof
  for (int w = 0; w < 3; ++w) P.dof_ops[w] = 0u;
  // (one owner per dof: two movable frames on one q_index -- a mimic-style table -- would OR two op indices into the field
  // and the quad kernel would read the joint record of a third frame; the Jacobian columns assume a single owner anyway)
  {
    uint32_t owned = 0u;
    for (int k = 0; k < F; ++k)
      if (P.ops[k].qidx >= 0 && P.ops[k].jtype != RMP2_JOINT_FIXED) {
        if ((owned >> P.ops[k].qidx) & 1u)
          return err = "q_index " + std::to_string(P.ops[k].qidx) + " is driven by more than one movable joint (mimic joints are not supported)",
                 RMP2_ERR_UNSUPPORTED;
        owned |= 1u << P.ops[k].qidx;
        P.dof_ops[P.ops[k].qidx / 6] |= (uint32_t)k << (5 * (P.ops[k].qidx % 6));
      }
  }
  P.n_id_leaves = nid;
  return RMP2_OK;
}


template <int N, int SLOTS, bool STRICT>
void launch_step(const rmp2_handle* h, const float* q, const float* qd, const float* goal, int gs, const ObsArgs& o,
                 const OutArgs& out, int R, hipStream_t s) {
  const int blocks = (R + kWave - 1) / kWave;
  h->last_kernel = STRICT ? "rmp2_step_kernel<STRICT> (one lane per robot, Jacobi pseudo-inverse)"
                          : "rmp2_step_kernel (one lane per robot)";
  if (h->has_point || o.capsule)
    RMP2_STEP_LAUNCH(h, (rmp2_step_kernel<N, SLOTS, STRICT, true>), dim3(blocks), dim3(kWave), 0, s, h->d_prog, q, qd, goal, gs,
                     o, out, R);
  else
    RMP2_STEP_LAUNCH(h, (rmp2_step_kernel<N, SLOTS, STRICT, false>), dim3(blocks), dim3(kWave), 0, s, h->d_prog, q, qd, goal, gs,
                     o, out, R);
}

template <int N, bool STRICT>
int dispatch_slots(const rmp2_handle* h, const float* q, const float* qd, const float* goal, int gs, const ObsArgs& o,
                   const OutArgs& out, int R, hipStream_t s) {
  with_slots(h->n_slots, [&](auto S) { launch_step<N, S, STRICT>(h, q, qd, goal, gs, o, out, R, s); });
  return RMP2_OK;
}

// the quad mapping's launchers (rmp2_quad_tu.hip), [N == 9][save slots]
constexpr decltype(&launch_quad_n9_s0) kLaunchQuad[2][3] = {{launch_quad_n2_s0, launch_quad_n2_s1, launch_quad_n2_s2},
                                                            {launch_quad_n9_s0, launch_quad_n9_s1, launch_quad_n9_s2}};

template <int N>
int dispatch_solve(const rmp2_handle* h, const float* q, const float* qd, const float* goal, int gs, const ObsArgs& o,
                   const OutArgs& out, const RolloutArgs& ro, int R, hipStream_t s) {
  const bool rollout = ro.n_iters != 1 || ro.substeps != 0;
  // RMP sets without any identity-map leaf carrying a positive diagonal metric (JointDamping, CSpaceBiasing,
  // ConfigurationSpaceBiasing) are rank deficient by construction on redundant arms (e.g. a lone target policy:
  // rank <= 3 of 9): every robot would fall through to the pseudo-inverse anyway, so AUTO goes there directly
  // (register-resident Jacobi, same result).
  const bool hex_forced = h->kernel_choice == 3;
  // ... except on 2-dof robots, where the fall-through of a flagged robot is a 2 x 2 Jacobi: there the elimination
  // mappings (with their split pair loops and culling) keep sets without an inertia leaf, e.g. the TwoJoint half of the
  // mixed fleet (config 5)
  // (solve = PINV on 2-dof robots takes the same mappings since round 4: the quad mapping's closed-form 2 x 2 resolve IS the
  // pseudo-inverse with TensorFlow's cutoff, for every robot, and the hex mapping's strict form is its careful path's; the
  // lane-per-robot strict kernel remains behind RMP2_KERNEL=lane)
  const bool cheap_fallthrough = N == 2 && h->kernel_choice != 1;
  // solve = PINV on a set whose metric is symmetric and carries an inertia leaf: the quad mapping's elimination CERTIFIES full
  // rank per robot (rmp2_quad.h, hdr.strict) -- where every singular value lies above TensorFlow's cutoff pinv(M) IS inv(M) --
  // and only uncertified robots take the Jacobi pseudo-inverse (its careful pass).  One launch, the AUTO step's cost, the
  // reference's semantics; at every fleet size and inside the fused rollout.
  const bool quad_certifies = quad_certifies_strict(h) && N == 9 && h->kernel_choice != 1 && !hex_forced;
  // (link geometry inside the step exists in the quad mapping only: such calls go there, flagged robots through its careful pass)
  if ((h->strict || h->likely_singular) && !rollout && !hex_forced && !cheap_fallthrough && !quad_certifies && !o.link_caps) {
    // Two kernels -- the quad mapping up to the combined metric and force (its pair loops are culled and split four ways;
    // the latency build for small grids), then rmp2_pinv_kernel, a lane per robot.  The lane-per-robot step kernel with the
    // same resolve keeps what the quad mapping does not carry (attached-point leaves, debug outputs, RMP2_KERNEL=lane).
    // (a caller who asks for the combined metric / force -- debug outputs, robot index slowest -- gets the lane kernel)
    // (attached-point sets included: their quad builds stop behind the combined system like the others; RMP2_KERNEL=quad asks
    // for exactly this path; debug outputs are copied out of the exchange buffer afterwards)
    if (N == 9 && (h->kernel_choice == 0 || h->kernel_choice == 2) && h->d_system && (size_t)R <= h->system_robots &&
        h->goal_floats <= 16 && !o.link_caps) {
      const int n = h->n_dof;
      OutArgs o2 = out;
      o2.M = h->d_system;                       // [n * n][R], robot index fastest
      o2.f = h->d_system + (size_t)R * n * n;   // [n][R]
      rmp2_handle* hm = const_cast<rmp2_handle*>(h);  // (the handle is the caller's mutable object: step_impl)
      void* const fence = hm->step_fence;
      hm->step_fence = nullptr;        // the completion fence belongs to the LAST kernel of the step
      hm->quad_skip_resolve = true;
      with_slots(h->n_slots, [&](auto S) { kLaunchQuad[1][S](h, q, qd, goal, gs, o, o2, ro, R, s); });
      hm->quad_skip_resolve = false;
      hm->step_fence = fence;
      if (out.M || out.f)
        hipLaunchKernelGGL(rmp2_system_copy_kernel, dim3((R + kWave - 1) / kWave), dim3(kWave), 0, s, o2.M, o2.f, out.M, out.f, n, R);
      RMP2_STEP_LAUNCH(h, (rmp2_pinv_kernel<9>), dim3((R + kWave - 1) / kWave), dim3(kWave), 0, s, o2.M, o2.f, out.qdd, out.status, n, R);
      hm->last_kernel_text = "rmp2_step_quad_kernel up to (M, f) + rmp2_pinv_kernel (one lane per robot, Jacobi pseudo-inverse) " + h->quad_build;
      h->last_kernel = h->last_kernel_text.c_str();  // (the tag: the instantiation the quad half ran, rmp2_host.h quad_build_tag)
      return RMP2_OK;
    }
    return dispatch_slots<N, true>(h, q, qd, goal, gs, o, out, R, s);
  }
  // Kernel choice (all mappings produce the same numbers to fp32 rounding):
  //  * hex (16 lanes per robot, rmp2_hex.h): the latency build -- fleets up to 8 192 robots, where the other mappings
  //    leave SIMDs idle; every leaf kind, both resolves, robots with up to 16 dofs; carries the fused rollout loop;
  //  * quad (4 lanes per robot, rmp2_quad.h): the throughput build for sets with distance leaves (the pair loops split
  //    4 ways); carries the fused rollout loop; no attached-point leaves;
  //  * lane-per-robot (this file): no redundant per-lane work -- large fleets without distance leaves; the strict
  //    pseudo-inverse (register-resident Jacobi) and attached-point leaves at any fleet size.
  // hex carries every leaf kind and both resolves (strict: the pseudo-inverse on every robot through its careful path;
  // slower than the lane kernel's register-resident Jacobi, so that path is taken on request / for n_dof > 9 only)
  // (link geometry of distance leaves: quad mapping only; attached-point leaves fed from a table + link capsules: hex too, for
  // sets without distance leaves -- its attached-point build stages no capsule table)
  const bool hex_ok = h->goal_floats <= 16 && (!o.link_caps || (h->has_point && !h->has_distance));
  // measured (bench.py, us per step, round 2 kernels; profiles/r02_dispatch_sweep.txt):
  //   cluttered set (config 3)   R:  4096   8192  10240  16384  20480  32768
  //     hex                         19.0   22.2   36.6   42.2   55.4   81.3
  //     quad                        29.0   30.6   30.7   31.0   35.6   35.1
  //   3-leaf set (config 2)      R:  4096   8192  10240  16384  32768  40960  65536  131072
  //     hex                          7.6    8.9   14.0   16.7   31.0
  //     quad                        13.0   13.6   14.0   13.9   16.8   25.7   31.0   68.5
  //     lane                        19.4   19.4   19.5   19.5   20.3   20.3   21.5   39.4
  // (hex holds two waves per SIMD: beyond 8 192 robots it runs a second round.)  Attached-point leaves exist in the hex
  // and lane mappings only: those sets keep the older hex / lane cut at 20 480 robots.  2-dof robots used to as well; with
  // the quad mapping's closed-form 2 x 2 resolve and 80-register builds the cut is the same 8 192 (round 3,
  // profiles/r03_dispatch_sweep.txt, TwoJoint half of config 5 with ragged lists, us per step):
  //     R:    4096   8192  12288  16384  20480  32768  65536
  //     hex    9.0   10.1   12.0   17.1   18.9   27.7   52.5
  //     quad  11.3   11.9   11.9   12.3   12.2   12.4   15.5
  // Attached-point leaves (round 3: carried by the quad mapping too, per-pair Jacobians collapsed into one pull-back per
  // frame) -- quad at every fleet size (profiles/r03_dispatch_sweep.txt, exp-05 set on the Panda, 4 pairs per leaf, us per step):
  //     R:    4096  16384  20480  32768  65536
  //     hex   33.3   80.3  102.8  155.0  301.5
  //     quad  26.3   28.6   33.5   58.3   90.8
  //     lane  79.7   80.6   83.8   88.9  105.1
  const int hex_max = h->has_point ? 0 : 8192;
  // the fused rollout of a solve = PINV handle (the reference's only resolve, rmp.py:153-154, inside the closed loop): the hex
  // mapping carries the strict pseudo-inverse through its careful path at any fleet size
  // (2-dof robots with link geometry on their distance leaves, which the hex mapping does not carry: the quad mapping, whose
  //  closed-form 2 x 2 resolve IS the pseudo-inverse for every robot, inside the rollout as in the plain step)
  const bool strict_rollout = h->strict && rollout && !quad_certifies && !(N == 2 && !hex_ok);
  // (the hex mapping certifies too since round 4 -- its Gauss-Jordan keeps the pivot rows --: strict small fleets take it like AUTO ones)
  // (2-dof robots under solve = PINV without a certificate -- sets without an inertia leaf, e.g. the TwoJoint half of config 5: the hex
  //  mapping resolves every robot through its careful path, the quad mapping by its closed-form 2 x 2 pseudo-inverse -- measured 14.3 us
  //  against ~12 at 4 096 robots (profiles/r05_cost_calibration.json): such calls take the quad mapping at every fleet size)
  const bool quad_closed_form = N == 2 && h->strict && !hex_certifies_strict(h) && !rollout;
  if (hex_ok && (h->kernel_choice == 3 || strict_rollout || (h->kernel_choice == 0 && R <= hex_max && !quad_closed_form && (!quad_certifies || hex_certifies_strict(h)))) &&
      (N == 2 ? launch_hex_n2 : launch_hex_n9)(h, q, qd, goal, gs, o, out, ro, R, s))
    return RMP2_OK;
  if (strict_rollout) return RMP2_ERR_UNSUPPORTED;  // (an uncertifying quad resolve would be AUTO: never a silent change of semantics)
  // (attached-point leaves: hex up to 20 480 robots, the quad mapping beyond -- round 3; the lane mapping on request)
  // (lane-per-robot beyond 49 152 robots without distance leaves -- round 5, config 2, us per step, quad | lane: 32 784 robots 16.5 | 21.8,
  //  65 536: 25.4 | 22.6, 131 072: 43.8 | 41.8 (profiles/r05_dispatch_lane_quad.txt) --, and only for solve = AUTO: a solve = PINV handle
  //  that reaches this point is one the quad mapping certifies, and the lane kernel's plain elimination would be AUTO's resolve under a
  //  PINV handle -- the same numbers on full-rank robots, but not what was asked for; until round 5 such fleets silently took it)
  const bool lane = !rollout && !o.link_caps && (h->kernel_choice == 1 ||
                                 (h->kernel_choice == 0 && !h->has_distance && !h->has_point && !h->strict && R > 49152));
  if (lane) return dispatch_slots<N, false>(h, q, qd, goal, gs, o, out, R, s);
  with_slots(h->n_slots, [&](auto S) { kLaunchQuad[N == 9][S](h, q, qd, goal, gs, o, out, ro, R, s); });
  return RMP2_OK;
}

// Pairs a stage wrote, described as EXPLICIT_PAIRS in `out`: leaves[i] (descriptor indices, ascending) owns the next count(i) pairs,
// every other leaf none.
template <class Count>
void explicit_pairs(const std::vector<int>& leaves, Count count, float* p_link, float* p_obs, float* dist, rmp2_obstacles& out) {
  std::memset(&out, 0, sizeof(out));
  out.mode = RMP2_OBS_EXPLICIT_PAIRS;
  int acc = 0;
  for (int l = 0, i = 0; l <= RMP2_MAX_LEAVES; ++l) {
    out.pair_begin[l] = acc;
    if (i < (int)leaves.size() && leaves[i] == l) acc += (int)count(i++);
  }
  out.n_pairs = acc;
  out.p_link = p_link, out.p_obs = p_obs, out.dist = dist;
}

// The (leaf, B) list of the self-collision setters (include/rmp2.h rmp2_set_self_collision): each leaf a pair leaf, each B a frame or
// -1 (the base) and not the leaf's own frame, then check(k, ordinal, B) (RMP2_OK or a refusal); B frames grouped by ordinal, in the
// order given.
template <class Check>
int group_self_pairs(rmp2_handle* h, int32_t n_pairs, const int32_t* pairs, std::vector<std::vector<int>>& by_leaf, Check check) {
  const int F = h->n_frames, L = (int)h->pair_leaves.size();
  int ord_of_leaf[RMP2_MAX_LEAVES];
  for (int l = 0; l < RMP2_MAX_LEAVES; ++l) ord_of_leaf[l] = -1;
  for (int o = 0; o < L; ++o) ord_of_leaf[h->pair_leaves[o]] = o;
  by_leaf.assign(L, {});
  for (int k = 0; k < n_pairs; ++k) {
    const int leaf = pairs[2 * k], b = pairs[2 * k + 1];
    const int o = (leaf >= 0 && leaf < h->n_leaves) ? ord_of_leaf[leaf] : -1;
    if (o < 0)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, "self pair " + std::to_string(k) + ": leaf " + std::to_string(leaf) +
                                                    " is not a distance or attached-point leaf");
    if (b < -1 || b >= F)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, "self pair " + std::to_string(k) + ": frame B " + std::to_string(b) + " out of range");
    if (b == h->pair_leaf_frame[o])
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, "self pair " + std::to_string(k) + ": frame B is the leaf's own frame");
    if (int rc = check(k, o, b)) return rc;
    by_leaf[o].push_back(b);
  }
  return RMP2_OK;
}

}  // namespace

// =========================================================================================
// device: inverse dynamics (rmp2_inverse_dynamics; the walk is rmp2_dynamics.h inverse_dynamics_robot)
// =========================================================================================
namespace {

// One lane per robot over the UNPRUNED program (the step's pruned program drops frames without a leaf, which still carry mass);
// the ops and the inertial records are read at wave-uniform addresses.  N: the handle's template size (dofs), SLOTS: the save
// slots of the unpruned program.
template <int N, int SLOTS>
__global__ void __launch_bounds__(kWave)
rmp2_inverse_dynamics_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, float ax, float ay, float az,
                             const float* __restrict__ q, const float* __restrict__ qd, const float* __restrict__ qdd,
                             float* __restrict__ tau, int R) {
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  const int n_dof = prog->n_dof;
  const size_t row = (size_t)robot * n_dof;
  const float base_acc[3] = {ax, ay, az};
  inverse_dynamics_robot<N, SLOTS>(prog->ops, prog->n_ops, n_dof, inert, base_acc, q + row, qd + row, qdd + row, tau + row);
}

template <int N>
void launch_inverse_dynamics(const rmp2_handle* h, const float* q, const float* qd, const float* qdd, float* tau, int R,
                             hipStream_t s) {
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  with_slots(h->n_slots_full, [&](auto S) {
    hipLaunchKernelGGL((rmp2_inverse_dynamics_kernel<N, S>), grid, block, 0, s, h->d_prog_full, h->d_inert, a[0], a[1], a[2], q, qd,
                       qdd, tau, R);
  });
}

}  // namespace

// =========================================================================================
// device: the plant (rmp2_mass_matrix / rmp2_forward_dynamics / rmp2_dynamics_step; the routines are rmp2_forward_dynamics.h)
// =========================================================================================
namespace {

// As the inverse dynamics: one lane per robot over the unpruned program, ops and inertial records at wave-uniform addresses.
template <int N, int SLOTS>
__global__ void __launch_bounds__(kWave)
rmp2_mass_matrix_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, const float* __restrict__ q,
                        float* __restrict__ M, int R) {
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  const int n_dof = prog->n_dof;
  mass_matrix_robot<N, SLOTS>(prog->ops, prog->n_ops, n_dof, inert, q + (size_t)robot * n_dof, M + (size_t)robot * n_dof * n_dof);
}

// rmp2_forward_dynamics (integrate = 0: one evaluation, q and qd only read) and rmp2_dynamics_step (the substep loop with the
// state in registers) in one kernel.
template <int N, int SLOTS>
__global__ void __launch_bounds__(kWave)
rmp2_dynamics_step_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, float ax, float ay, float az,
                          float* q, float* qd, const float* __restrict__ u, int accel, const float* __restrict__ lim, float dt,
                          int substeps, int integrate, float* __restrict__ qdd_out, float* __restrict__ tau_out, int R) {
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  const int n_dof = prog->n_dof;
  const size_t row = (size_t)robot * n_dof;
  const float base_acc[3] = {ax, ay, az};
  dynamics_step_robot<N, SLOTS>(prog->ops, prog->n_ops, n_dof, inert, base_acc, q + row, qd + row, u + row, accel != 0, lim, dt,
                                substeps, integrate != 0, qdd_out ? qdd_out + row : nullptr, tau_out ? tau_out + row : nullptr);
}

template <int N>
void launch_mass_matrix(const rmp2_handle* h, const float* q, float* M, int R, hipStream_t s) {
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  with_slots(h->n_slots_full, [&](auto S) {
    hipLaunchKernelGGL((rmp2_mass_matrix_kernel<N, S>), grid, block, 0, s, h->d_prog_full, h->d_inert, q, M, R);
  });
}

template <int N>
void launch_dynamics_step(const rmp2_handle* h, float* q, float* qd, const float* u, int accel, const float* lim, float dt,
                          int substeps, int integrate, float* qdd_out, float* tau_out, int R, hipStream_t s) {
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  with_slots(h->n_slots_full, [&](auto S) {
    hipLaunchKernelGGL((rmp2_dynamics_step_kernel<N, S>), grid, block, 0, s, h->d_prog_full, h->d_inert, a[0], a[1], a[2], q, qd, u,
                       accel, lim, dt, substeps, integrate, qdd_out, tau_out, R);
  });
}

// The refusals the plant's steps share.  step_args_check: the drive, substeps and dt of rmp2_dynamics_step /
// rmp2_dynamics_step_stops.  step_rows_check: R, the inertial table and the arrays every call needs; launch = false: R == 0, no-op.
int step_args_check(rmp2_handle* h, const char* what, int drive, int substeps, float dt) {
  if (drive != RMP2_DRIVE_TORQUE && drive != RMP2_DRIVE_ACCEL)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown drive " + std::to_string(drive));
  if (substeps < 1) return fail(h, RMP2_ERR_INVALID_ARGUMENT, std::string(what) + ": substeps < 1");
  if (!std::isfinite(dt) || !(dt > 0.f)) return fail(h, RMP2_ERR_INVALID_ARGUMENT, std::string(what) + ": dt must be finite and > 0");
  return RMP2_OK;
}

int step_rows_check(rmp2_handle* h, const char* what, const float* q, const float* qd, const float* u, bool others_ok, int R,
                    bool& launch) {
  launch = false;
  if (R < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, std::string(what) + ": R < 0");
  if (h->inert_n == 0)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, std::string(what) + ": no inertial table on this handle (call rmp2_set_inertials first)");
  if (R == 0) return RMP2_OK;
  if (!q || !qd || !u || !others_ok) return fail(h, RMP2_ERR_INVALID_ARGUMENT, std::string(what) + ": null array");
  launch = true;
  return use_device(h);
}

int dynamics_step_impl(rmp2_handle* h, const char* what, float* q, float* qd, const float* u, int accel, const float* lim, float dt,
                       int substeps, int integrate, float* qdd_out, float* tau_out, int R, void* stream) {
  bool launch;
  if (int rc = step_rows_check(h, what, q, qd, u, integrate || qdd_out, R, launch)) return rc;
  if (!launch) return RMP2_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (h->n_template) {
    case 2: launch_dynamics_step<2>(h, q, qd, u, accel, lim, dt, substeps, integrate, qdd_out, tau_out, R, s); break;
    case 9: launch_dynamics_step<9>(h, q, qd, u, accel, lim, dt, substeps, integrate, qdd_out, tau_out, R, s); break;
    default: launch_dynamics_step<16>(h, q, qd, u, accel, lim, dt, substeps, integrate, qdd_out, tau_out, R, s); break;
  }
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

// rmp2_dynamics_step_stops: the step with joint-limit stops (the kernel and its routines are rmp2_joint_stops.h)
template <int N>
void launch_dynamics_step_stops(const rmp2_handle* h, float* q, float* qd, const float* u, int accel, const float* lim,
                                const float* qlo, const float* qhi, float dt, int substeps, float* qdd_out, float* tau_out,
                                float* stop_out, uint32_t* status_out, int R, hipStream_t s) {
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  with_slots(h->n_slots_full, [&](auto S) {
    hipLaunchKernelGGL((rmp2_dynamics_step_stops_kernel<N, S>), grid, block, 0, s, h->d_prog_full, h->d_inert, a[0], a[1], a[2], q,
                       qd, u, accel, lim, qlo, qhi, dt, substeps, qdd_out, tau_out, stop_out, status_out, R);
  });
}

// The contact step's launchers (rmp2_contacts_tu.hip; the kernels and their routines are rmp2_contacts.h): [kernel family][LIST],
// the families in the order each adds to the one before -- spheres, planes, capsules, self, cylinders, cylinder lists
constexpr ContactLauncher* kLaunchContacts[6][2] = {{launch_contacts_table, launch_contacts_lists},
                                                    {launch_contacts_table_planes, launch_contacts_lists_planes},
                                                    {launch_contacts_table_capsules, launch_contacts_lists_capsules},
                                                    {launch_contacts_table_self, launch_contacts_lists_self},
                                                    {launch_contacts_table_cylinders, launch_contacts_lists_cylinders},
                                                    {launch_contacts_table_cylinder_lists, launch_contacts_lists_cylinder_lists}};

// The host path of the seven contact entry points.  form: which of them is calling -- the checks are shared and run in one order;
// each entry point keeps its `what` and its own rules (table: K <= RMP2_MAX_CONTACT_SPHERES; lists: both CSR arrays, the pool
// aligned; planes: the CSR arrays both set or both null, P and the plane table; capsules: the planes' rules, C and the capsule
// table; self: the capsules' rules, the pairs are the handle's).  The planes entry always runs a PLANES kernel, P == 0 included;
// the capsules entry always a capsule kernel (planes and capsules on), P == 0 and C == 0 included; the self entry always a self
// kernel (planes, capsules and self on), no pairs set included; the cylinders entry (the self call's rules, Y, the cylinder table
// and the self_pairs flag) always a cylinder kernel, Y == 0 included; the cylinder-lists entry (the cylinders call's rules with the
// pool's cap on Y, and both cylinder CSR arrays) always a cylinder-list kernel.
enum ContactForm {
  kContactsTable, kContactsLists, kContactsPlanes, kContactsCapsules, kContactsSelf, kContactsCylinders, kContactsCylinderLists
};

// The fields every contact entry point has, in the order its parameter list has them; the rest off (no lists, no tables, the
// handle's self pairs on) for the entry to set by name.
ContactCall contact_call(float* q, float* qd, const float* u, const float* tau_limit, const float* q_lower, const float* q_upper,
                         const float* spheres, int32_t K, float d_act, float dt, int32_t substeps, float* qdd_out, float* tau_out,
                         float* stop_out, float* contact_out, float* contact_lambda, int32_t* contact_pair, uint32_t* status_out,
                         int32_t R) {
  ContactCall c{};
  c.q = q, c.qd = qd, c.u = u, c.lim = tau_limit, c.qlo = q_lower, c.qhi = q_upper;
  c.spheres = spheres, c.K = K, c.d_act = d_act, c.dt = dt, c.substeps = substeps, c.self_pairs = 1;
  c.qdd_out = qdd_out, c.tau_out = tau_out, c.stop_out = stop_out, c.contact_out = contact_out, c.lambda_out = contact_lambda;
  c.pair_out = contact_pair, c.status_out = status_out, c.R = R;
  return c;
}

// c: the call as its entry point filled it (contact_call and the entry's own fields), accel apart, which follows drive here.
int contacts_step_impl(rmp2_handle* h, const char* what, ContactForm form, int32_t drive, ContactCall c, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  const std::string w = what;
  if (int rc = step_args_check(h, what, drive, c.substeps, c.dt)) return rc;
  const bool cylinder_lists = form == kContactsCylinderLists;   // (the cylinders call's rules; the pool's cap on Y)
  const bool with_cylinders = form == kContactsCylinders || cylinder_lists;   // (the self call's rules; always a cylinder kernel, Y == 0 included)
  const bool with_self = form == kContactsSelf || with_cylinders;   // (the capsules' rules; always a self kernel, no pairs set included)
  const bool with_capsules = form == kContactsCapsules || with_self;
  const bool with_planes = form == kContactsPlanes || with_capsules;
  if (with_planes && (c.csr_offset != nullptr) != (c.csr_index != nullptr))
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": csr_offset and csr_index go together (both null: the shared table)");
  const bool lists = form == kContactsLists || (with_planes && c.csr_offset);
  const int k_max = lists ? RMP2_MAX_CONTACT_POOL : RMP2_MAX_CONTACT_SPHERES;
  if (c.K < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": K < 0");
  if (c.K > k_max) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": K > " + std::to_string(k_max));
  if (lists && c.K > 0 && c.spheres && ((uintptr_t)c.spheres & 15u))
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": the pool must be 16-byte aligned");
  if (with_planes) {
    if (c.P < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": P < 0");
    if (c.P > RMP2_MAX_CONTACT_PLANES)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": P > " + std::to_string(RMP2_MAX_CONTACT_PLANES));
    if (c.P > 0 && !c.planes) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": null plane table with P > 0");
    if (c.P > 0 && ((uintptr_t)c.planes & 15u))
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": the plane table must be 16-byte aligned");
  }
  if (with_capsules) {
    if (c.C < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": C < 0");
    if (c.C > RMP2_MAX_OBSTACLE_CAPSULES)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": C > " + std::to_string(RMP2_MAX_OBSTACLE_CAPSULES));
    if (c.C > 0 && !c.capsules) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": null capsule table with C > 0");
    if (c.C > 0 && ((uintptr_t)c.capsules & 15u))
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": the capsule table must be 16-byte aligned");
  }
  if (with_cylinders) {
    if (c.Y < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": Y < 0");
    const int y_max = cylinder_lists ? RMP2_MAX_CYLINDER_POOL : RMP2_MAX_OBSTACLE_CYLINDERS;
    if (c.Y > y_max) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": Y > " + std::to_string(y_max));
    const std::string table = cylinder_lists ? "cylinder pool" : "cylinder table";
    if (c.Y > 0 && !c.cylinders) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": null " + table + " with Y > 0");
    if (c.Y > 0 && ((uintptr_t)c.cylinders & 15u))
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": the " + table + " must be 16-byte aligned");
    if (c.self_pairs != 0 && c.self_pairs != 1) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": self_pairs must be 0 or 1");
  }
  if (!std::isfinite(c.d_act) || c.d_act < 0.f) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": d_act must be finite and >= 0");
  if (h->contact_n == 0)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": no contact capsules on this handle (call rmp2_set_contact_capsules first)");
  if (h->n_template > 9)
    return fail(h, RMP2_ERR_UNSUPPORTED,
                w + ": robots of more than 9 dofs are not supported (this one has " + std::to_string(h->n_dof) + ")");
  bool launch;
  const bool others_ok = (c.qlo != nullptr) == (c.qhi != nullptr) && (c.K == 0 || c.spheres) &&
                         (form != kContactsLists || (c.csr_offset && c.csr_index)) && (!cylinder_lists || (c.cyl_offset && c.cyl_index));
  if (int rc = step_rows_check(h, what, c.q, c.qd, c.u, others_ok, c.R, launch)) return rc;
  if (!launch) return RMP2_OK;
  // (N in {2, 9} by the handle's template size, SLOTS by its program)
  c.accel = drive == RMP2_DRIVE_ACCEL;
  static_assert(kContactsPlanes + 1 == kContactsCapsules && kContactsCapsules + 1 == kContactsSelf && kContactsSelf + 1 == kContactsCylinders &&
                    kContactsCylinders + 1 == kContactsCylinderLists && kContactsCylinderLists - kContactsPlanes + 1 == 5,
                "the forms from kContactsPlanes on stand in the order of kLaunchContacts' rows 1 .. 5");
  kLaunchContacts[with_planes ? form - kContactsPlanes + 1 : 0][lists](h, c, (hipStream_t)stream);
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

int rmp2_abi_version(void) { return RMP2_ABI_VERSION; }
size_t rmp2_sizeof_desc(void) { return sizeof(rmp2_desc); }
size_t rmp2_sizeof_obstacles(void) { return sizeof(rmp2_obstacles); }

const char* rmp2_last_error(const rmp2_handle* h) { return h ? h->error.c_str() : g_create_error.c_str(); }

const char* rmp2_last_kernel(const rmp2_handle* h) { return h ? h->last_kernel : "none"; }

// ---- device-scope fences (include/rmp2.h) ---------------------------------------------------------------------------
int rmp2_fence_create(int device, void** fence) {
  if (!fence) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "null argument");
  *fence = nullptr;
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) return fail(nullptr, RMP2_ERR_HIP, "hipGetDevice failed");
  if (prev != device && hipSetDevice(device) != hipSuccess) return fail(nullptr, RMP2_ERR_HIP, "hipSetDevice failed");
  hipEvent_t ev = nullptr;
  const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventDisableSystemFence);
  if (prev != device) (void)hipSetDevice(prev);
  if (e != hipSuccess) return fail(nullptr, RMP2_ERR_HIP, std::string("hipEventCreateWithFlags: ") + hipGetErrorString(e));
  *fence = ev;
  return RMP2_OK;
}
int rmp2_fence_record(void* fence, void* stream) {
  if (!fence) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "null fence");
  const hipError_t e = hipEventRecord(static_cast<hipEvent_t>(fence), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? RMP2_OK : fail(nullptr, RMP2_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
}
int rmp2_fence_wait(void* fence, void* stream) {
  if (!fence) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "null fence");
  const hipError_t e = hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(fence), 0);
  return e == hipSuccess ? RMP2_OK : fail(nullptr, RMP2_ERR_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
}
int rmp2_set_step_fence(rmp2_handle* h, void* fence) {
  if (!h) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "null handle");
  std::lock_guard<std::mutex> lock(g_fence_mutex);
  if (h->step_fence) {
    auto it = g_attached_fences.find(h->step_fence);
    if (it != g_attached_fences.end() && --it->second == 0) g_attached_fences.erase(it);
  }
  h->step_fence = fence;
  if (fence) ++g_attached_fences[fence];
  return RMP2_OK;
}
int rmp2_fence_destroy(void* fence) {
  if (!fence) return RMP2_OK;
  {
    std::lock_guard<std::mutex> lock(g_fence_mutex);
    if (g_attached_fences.count(fence))
      return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT,
                  "fence is still attached to a handle (rmp2_set_step_fence): detach it (NULL) or destroy the handle first");
  }
  return hipEventDestroy(static_cast<hipEvent_t>(fence)) == hipSuccess ? RMP2_OK : fail(nullptr, RMP2_ERR_HIP, "hipEventDestroy failed");
}

int rmp2_leaf_evaluate(int device, const rmp2_leaf* leaf, int32_t k, const float* x, const float* xd, const float* goal,
                       const float* dist, const float* nvec, float* xdd, float* A, int32_t B, void* stream) {
  if (!leaf || !x || !xd || !xdd || !A || B < 0) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "null argument");
  int want = -1;  // task-space dimension the leaf kind fixes (-1: any 1 .. RMP2_MAX_DOF)
  bool needs_goal = false, needs_pairs = false;
  switch (leaf->kind) {
    case RMP2_LEAF_TARGET_ATTRACTOR: want = 3, needs_goal = true; break;
    case RMP2_LEAF_OBSTACLE_AVOIDANCE: want = 1; break;
    case RMP2_LEAF_COLLISION_AVOIDANCE: want = 3, needs_pairs = true; break;
    case RMP2_LEAF_TARGET_POLICY: needs_goal = true; break;
    case RMP2_LEAF_JOINT_VELOCITY_CAP: case RMP2_LEAF_JOINT_DAMPING: case RMP2_LEAF_CSPACE_BIASING:
    case RMP2_LEAF_JOINT_LIMIT_AVOIDANCE: case RMP2_LEAF_CONFIG_SPACE_BIASING: break;
    default: return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "unknown leaf kind");
  }
  if (k < 1 || k > RMP2_MAX_DOF || (want > 0 && k != want))
    return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "task-space dimension does not fit this leaf kind");
  if (needs_goal && !goal) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "this leaf needs a goal");
  if (needs_pairs && (!dist || !nvec)) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "CollisionAvoidance needs dist and nvec");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
    return fail(nullptr, RMP2_ERR_NO_DEVICE, "no usable HIP device (this library has no CPU path)");
  if (B == 0) return RMP2_OK;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != device) HIP_TRY(nullptr, hipSetDevice(device));
  hipLaunchKernelGGL(rmp2_leaf_kernel, dim3((B + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream, *leaf, k, x, xd,
                     goal, dist, nvec, xdd, A, B);
  HIP_TRY(nullptr, hipGetLastError());
  return RMP2_OK;
}

// The descriptor checks of rmp2_validate and rmp2_create: the step's pruned program P (and the hex kernel's ops) and the unpruned
// program Pfull compile, and fit the kernels' limits.
static int compile_desc(const rmp2_desc& d, DevProgram& P, int& n_slots, DevProgram& Pfull, int& n_slots_full, std::vector<HexOp>& hops) {
  std::string err;
  int rc = compile_program(d, P, n_slots, err, /*prune=*/true, &hops);
  if (rc == RMP2_OK) rc = compile_program(d, Pfull, n_slots_full, err, /*prune=*/false);
  if (rc != RMP2_OK) return fail(nullptr, rc, err);
  // 10 .. 16 dofs: the hex kernel (one metric row per lane, 16 lanes per robot) is the only mapping instantiated; it carries every
  // leaf kind and both resolves
  if (d.robot.n_dof > 9 && d.goal_floats > 16)
    return fail(nullptr, RMP2_ERR_UNSUPPORTED, "more than 16 goal floats per robot with n_dof > 9");
  if (n_slots > 2 || n_slots_full > 2)   // (with_slots stops at 2)
    return fail(nullptr, RMP2_ERR_UNSUPPORTED, "kinematic tree needs more than 2 saved branch states");
  return RMP2_OK;
}

int rmp2_validate(const rmp2_desc* desc) {
  if (!desc) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "null argument");
  if (desc->abi_version != RMP2_ABI_VERSION)
    return fail(nullptr, RMP2_ERR_ABI_MISMATCH, "rmp2_desc.abi_version does not match the library");
  // (DevProgram is ~20 KB: on the heap, like rmp2_create's copies are short-lived stack objects of the same size)
  std::vector<DevProgram> P(2);
  int n_slots = 0, n_slots_full = 0;
  std::vector<HexOp> hops;
  return compile_desc(*desc, P[0], n_slots, P[1], n_slots_full, hops);
}

int rmp2_identity_records(const rmp2_desc* desc, void* records, int32_t capacity) {
  if (!desc || (capacity > 0 && !records)) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "null argument");
  if (desc->abi_version != RMP2_ABI_VERSION)
    return fail(nullptr, RMP2_ERR_ABI_MISMATCH, "rmp2_desc.abi_version does not match the library");
  std::vector<DevProgram> P(2);
  int n_slots = 0, n_slots_full = 0;
  std::vector<HexOp> hops;
  if (int rc = compile_desc(*desc, P[0], n_slots, P[1], n_slots_full, hops)) return rc;
  if (!P[0].id_structured) return 0;
  const int n = P[0].n_id_leaves;
  std::memcpy(records, P[0].id_recs, sizeof(IdLeafRec) * (size_t)std::max(0, std::min(n, (int)capacity)));
  return n;
}

int rmp2_create(const rmp2_desc* desc, int device, rmp2_handle** out) {
  if (!desc || !out) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (desc->abi_version != RMP2_ABI_VERSION)
    return fail(nullptr, RMP2_ERR_ABI_MISMATCH, "rmp2_desc.abi_version does not match the library");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
    return fail(nullptr, RMP2_ERR_NO_DEVICE, "no usable HIP device (this library has no CPU path)");
  DevProgram P, Pfull;
  int n_slots = 0, n_slots_full = 0;
  std::vector<HexOp> hops;
  if (int rc = compile_desc(*desc, P, n_slots, Pfull, n_slots_full, hops)) return rc;
  rmp2_handle* h = new (std::nothrow) rmp2_handle();
  if (!h) return fail(nullptr, RMP2_ERR_HIP, "out of host memory");
  h->device = device;
  h->n_dof = desc->robot.n_dof;
  h->n_frames = desc->robot.n_frames;
  h->n_slots = n_slots;
  h->n_slots_full = n_slots_full;
  h->n_ops_step = P.n_ops;
  h->n_leaves = desc->n_leaves;
  h->goal_floats = desc->goal_floats;
  h->n_template = h->n_dof <= 2 ? 2 : (h->n_dof <= 9 ? 9 : 16);
  h->strict = desc->solve_mode == RMP2_SOLVE_PINV;
  h->n_id_leaves = P.n_id_leaves;
  h->id_structured = P.id_structured != 0;
  h->likely_singular = true;
  for (int l = 0; l < desc->n_leaves; ++l) {
    const rmp2_leaf& lf = desc->leaves[l];
    if (lf.taskmap != RMP2_TASKMAP_IDENTITY) continue;
    if ((lf.kind == RMP2_LEAF_JOINT_DAMPING && lf.params[2] > 0.f) ||
        (lf.kind == RMP2_LEAF_CSPACE_BIASING && lf.params[0] + lf.params[4] > 0.f) ||
        (lf.kind == RMP2_LEAF_CONFIG_SPACE_BIASING && lf.params[2] > 0.f))
      h->likely_singular = false;
  }
  h->symmetric = true;  // every kind but JointLimitAvoidance (A = w * H scales COLUMNS, quirk Q2) has a symmetric metric
  for (int l = 0; l < desc->n_leaves; ++l)
    if (desc->leaves[l].kind == RMP2_LEAF_JOINT_LIMIT_AVOIDANCE) h->symmetric = false;
#ifdef RMP2_TUNING  // A/B knobs of the tuning builds only (tools/): a stray variable must not change a deployment's dispatch
  if (const char* we = std::getenv("RMP2_PRIO_TAIL")) h->prio_tail = std::atoi(we) & 3;
  if (const char* we = std::getenv("RMP2_QUAD_LATENCY_BLOCKS")) h->quad_latency_blocks = std::atoi(we), h->quad_latency_set = true;
#endif
  if (const char* ce = std::getenv("RMP2_STRICT_CERTIFY")) h->strict_certify = std::atoi(ce) != 0;
  if (const char* ge = std::getenv("RMP2_EXPLICIT_GLDS")) h->explicit_glds = std::atoi(ge) != 0;
  if (const char* se = std::getenv("RMP2_EXPLICIT_STREAM")) h->explicit_stream = std::atoi(se) != 0 ? 1 : 0;
  if (const char* sg = std::getenv("RMP2_STREAM_STAGGER")) h->stream_stagger = std::max(0, std::min(1023, std::atoi(sg)));  // (bits 8-9: A/B switches of the stream, rmp2_quad.h pair_loop_explicit_glds)
  if (const char* we = std::getenv("RMP2_QUAD_SYM")) h->symmetric = h->symmetric && std::atoi(we) != 0;  // 0 = general form (include/rmp2.h)
  h->n_leaf_ops = P.n_leaf_ops;
  h->hex_levels = P.hex.n_levels;
  h->hex_waves = 4;
#ifdef RMP2_TUNING
  {
    const char* we = std::getenv("RMP2_HEX_WAVES");
    h->hex_waves = (we && std::atoi(we) == 1) ? 1 : 4;
  }
#endif
  {
    const char* we = std::getenv("RMP2_QUAD_MINW");
    const int wv = we ? std::atoi(we) : 0;
    h->quad_minw = (wv >= 2 && wv <= 4) ? wv : 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      h->n_simd = 4 * prop.multiProcessorCount;
    // The latency build (program staged in LDS, all registers; made for grids of at most one wave per SIMD) is retired from the
    // dispatch: on the round-5 kernels the throughput build is faster on every such grid -- config 3, 1 024 .. 16 384 robots: 27.1 ..
    // 29.4 us against 31.4 .. 33.4; config 2: 12.5 .. 13.5 against 13.6 .. 14.7 (profiles/r05_quad_latency_build_ab.txt).  It stays
    // compiled for the tuning builds' A/B (RMP2_QUAD_LATENCY_BLOCKS).
    if (!h->quad_latency_set) h->quad_latency_blocks = 0;
  }
  h->n_fk_leaves = P.n_fk_leaves;
  h->hex_is_chain = P.hex.is_chain;
  h->rev_mask = P.rev_mask;
  for (int w = 0; w < 3; ++w) h->dof_ops[w] = P.dof_ops[w];
  {
    const char* kenv = std::getenv("RMP2_KERNEL");
    h->kernel_choice = !kenv ? 0
                       : (std::strcmp(kenv, "lane") == 0 ? 1
                          : (std::strcmp(kenv, "quad") == 0 ? 2 : (std::strcmp(kenv, "hex") == 0 ? 3 : 0)));
  }
  for (int l = 0; l < desc->n_leaves; ++l)
    if (desc->leaves[l].taskmap == RMP2_TASKMAP_FK_DISTANCE) h->distance_leaves.push_back(l);
  h->has_distance = !h->distance_leaves.empty();
  {  // at most one FK_DISTANCE leaf per frame: the lean link-geometry builds carry one segment per leaf-bearing frame
    int per_frame[RMP2_MAX_FRAMES] = {};
    h->link_rows_ok = true;
    for (int l : h->distance_leaves)
      if (desc->leaves[l].frame >= 0 && desc->leaves[l].frame < RMP2_MAX_FRAMES && ++per_frame[desc->leaves[l].frame] > 1) h->link_rows_ok = false;
  }
  if (const char* le = std::getenv("RMP2_LINK_LEAN")) h->link_rows_ok = h->link_rows_ok && std::atoi(le) != 0;  // 0: attached-record builds (A/B)
  for (int l : h->distance_leaves)
    h->cull_c0 = std::max(h->cull_c0, desc->leaves[l].params[7] + desc->leaves[l].params[0]);
  for (int l = 0; l < desc->n_leaves; ++l)
    if (desc->leaves[l].taskmap == RMP2_TASKMAP_FK_POINT) h->has_point = true;
  for (int l = 0; l < desc->n_leaves; ++l)
    if (desc->leaves[l].taskmap == RMP2_TASKMAP_FK_DISTANCE || desc->leaves[l].taskmap == RMP2_TASKMAP_FK_POINT) {
      h->pair_leaves.push_back(l);
      h->pair_leaf_frame.push_back(desc->leaves[l].frame);
      h->pair_leaf_point.push_back(desc->leaves[l].taskmap == RMP2_TASKMAP_FK_POINT ? 1 : 0);
    }
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc(&h->d_prog, sizeof(DevProgram));
  if (e == hipSuccess) e = hipMemcpy(h->d_prog, &P, sizeof(DevProgram), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&h->d_prog_full, sizeof(DevProgram));
  if (e == hipSuccess) e = hipMemcpy(h->d_prog_full, &Pfull, sizeof(DevProgram), hipMemcpyHostToDevice);
  for (int k = 0; k < Pfull.n_ops; ++k) {   // (rmp2_set_contact_self_pairs: roles by op order, masks by ancestor dofs)
    h->full_op_frame.push_back(Pfull.ops[k].frame);
    h->full_op_anc.push_back(Pfull.ops[k].anc_mask & 0xffffu);   // (the dof set alone: bits 16 + j are structural_lever_zeros')
  }
  {
    // hex kernel: one contiguous blob = [HexCtl | HexOp | leaves in execution order | leaf-frame records | jump | op_anc]
    std::vector<unsigned char> blob;
    auto put = [&blob](const void* p, size_t n) {
      const unsigned char* b = static_cast<const unsigned char*>(p);
      blob.insert(blob.end(), b, b + n);
    };
    for (int k = 0; k < P.n_ops; ++k) {
      const DevOp& o = P.ops[k];
      const HexCtl c{o.jtype, o.qidx, o.anc_mask, o.leaf_begin, o.leaf_count, {o.axis[0], o.axis[1], o.axis[2]}};
      put(&c, sizeof(c));
    }
    put(hops.data(), sizeof(HexOp) * hops.size());
    // leaf records in EXECUTION order (FK leaves grouped by frame, then the identity-map leaves): the kernel
    // indexes them directly -- every indirection through a list is one more dependent LDS round trip per leaf
    for (int i = 0; i < P.n_fk_leaves; ++i) put(&P.leaves[P.fk_leaves[i]], sizeof(DevLeaf));
    for (int i = 0; i < P.n_id_leaves; ++i) put(&P.leaves[P.id_leaves[i]], sizeof(DevLeaf));
    // one 16-byte record per leaf-bearing frame: (op, ancestor dofs, first leaf, leaf count)
    for (int t = 0; t < P.n_leaf_ops; ++t) {
      const DevOp& o = P.ops[P.leaf_ops[t]];
      const int32_t rec[4] = {P.leaf_ops[t], (int32_t)o.anc_mask, o.leaf_begin, o.leaf_count};
      put(rec, sizeof(rec));
    }
    // int tables: jump[n_levels][n_ops] | op_anc[n_ops], padded to 16 bytes
    for (int l = 0; l < P.hex.n_levels; ++l) put(P.hex.jump[l], sizeof(int32_t) * P.n_ops);
    put(P.hex.op_anc, sizeof(uint32_t) * P.n_ops);
    while (blob.size() % 16) blob.push_back(0);
    h->hex_blob16 = (int)(blob.size() / 16);
    if (e == hipSuccess) e = hipMalloc(&h->d_hex_blob, blob.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_hex_blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMalloc(&h->d_pair_begin, sizeof(h->h_pair_begin));
  if (e == hipSuccess) e = hipMemset(h->d_pair_begin, 0, sizeof(h->h_pair_begin));
  if (e != hipSuccess) {
    const std::string msg = std::string("device setup failed: ") + hipGetErrorString(e);
    rmp2_destroy(h);
    return fail(nullptr, RMP2_ERR_HIP, msg);
  }
  *out = h;
  return RMP2_OK;
}

int rmp2_destroy(rmp2_handle* h) {
  if (!h) return RMP2_OK;
  rmp2_set_step_fence(h, nullptr);  // (a fence attached to a destroyed handle is free to be destroyed)
  int prev = -1;  // the caller's current device is left as it was
  if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  (void)hipSetDevice(h->device);
  if (h->d_prog) (void)hipFree(h->d_prog);
  if (h->d_prog_full) (void)hipFree(h->d_prog_full);
  if (h->d_hex_blob) (void)hipFree(h->d_hex_blob);
  if (h->d_pair_begin) (void)hipFree(h->d_pair_begin);
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  if (h->d_system) (void)hipFree(h->d_system);
  if (h->d_stage) (void)hipFree(h->d_stage);
  if (h->d_self) (void)hipFree(h->d_self);
  if (h->d_hull) (void)hipFree(h->d_hull);
  if (h->d_hull_verts) (void)hipFree(h->d_hull_verts);
  if (h->d_hull_planes) (void)hipFree(h->d_hull_planes);
  if (h->d_shull) (void)hipFree(h->d_shull);
  if (h->d_inert) (void)hipFree(h->d_inert);
  if (h->d_contact_caps) (void)hipFree(h->d_contact_caps);
  if (h->d_contact_self) (void)hipFree(h->d_contact_self);
  if (prev >= 0 && prev != h->device) (void)hipSetDevice(prev);
  delete h;
  return RMP2_OK;
}

// Whether the step itself forms the pairs of link geometry on `obs` (include/rmp2.h rmp2_obstacles.link_capsules): tables of at most
// 256 primitives, no CYLINDER, robots with at most 9 dofs and 16 goal floats, solve = pinv only where the quad mapping certifies or
// computes it.  Beyond, plain steps of distance-leaf sets are staged (stage_link_geometry) and the others refused (prepare_step).
static bool fused_link_geometry_fits(const rmp2_handle* h, const rmp2_obstacles* obs) {
  if (obs->n_spheres > kLdsSpheres || obs->primitive == RMP2_PRIM_CYLINDER || h->n_template > 9 || h->goal_floats > 16) return false;
  // (2-dof robots: the quad mapping's closed-form 2 x 2 resolve IS the pseudo-inverse with TensorFlow's cutoff, for every robot;
  // sets with attached-point leaves resolve as they do on explicit arrays: the rank-deficient ones through the careful pass)
  if (h->n_template == 2) return true;
  return !(h->strict && !quad_certifies_strict(h)) && (h->has_point || !h->likely_singular);
}

// Argument checks of a control step and the kernels' view of its obstacle / output arguments (R > 0).
static int prepare_step(rmp2_handle* h, const float* q, const float* qd, const float* goal, int32_t goal_stride,
                        const rmp2_obstacles* obs, const rmp2_outputs* out, const RolloutArgs& ro, int32_t R, void* stream,
                        ObsArgs& o, OutArgs& oa) {
  if (!q || !qd || !out || !out->qdd) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "q, qd and out->qdd are required");
  if (h->goal_floats > 0) {
    if (!goal) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "this RMP set has goal-bearing leaves: goal is required");
    if (goal_stride != 0 && goal_stride < h->goal_floats)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, "goal_stride must be 0 (shared) or >= goal_floats");
  }
  hipStream_t s = (hipStream_t)stream;
  if (int rc = use_device(h)) return rc;
  std::memset(&o, 0, sizeof(o));
  o.mode = obs ? obs->mode : RMP2_OBS_NONE;
  if (h->has_point) {
    // attached-point leaves read (relative_position, normal_vec, distance) per pair: from the caller's arrays, or -- a shared
    // primitive table plus link capsules -- formed inside the step from the closest points of link and primitive, per control
    // step (which is what lets such a set roll out: 05_obstacle_avoidance.py:51-72 re-feeds the Datamanager every step)
    const bool from_table = obs && obs->mode == RMP2_OBS_SHARED_SPHERES && obs->link_capsules;
    const bool rollout = ro.n_iters != 1 || ro.substeps != 0;
    if (rollout && !from_table)
      return fail(h, RMP2_ERR_UNSUPPORTED, "rollout: attached-point leaves take per-step pair data -- give a SHARED_SPHERES table "
                                           "with link_capsules instead of EXPLICIT_PAIRS arrays");
    if (!from_table && (o.mode != RMP2_OBS_EXPLICIT_PAIRS || !obs->dist))
      return fail(h, RMP2_ERR_INVALID_ARGUMENT,
                  "attached-point leaves need EXPLICIT_PAIRS data (p_link = relative_position, p_obs = normal_vec, dist) or a "
                  "SHARED_SPHERES table with link_capsules");
  }
  if (h->has_distance || h->has_point) {
    if (o.mode == RMP2_OBS_NONE)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, "this RMP set has distance leaves: obstacles are required");
    if (o.mode == RMP2_OBS_EXPLICIT_PAIRS) {
      if (!obs->p_link || !obs->p_obs || obs->n_pairs < 0)
        return fail(h, RMP2_ERR_INVALID_ARGUMENT, "EXPLICIT_PAIRS needs p_link, p_obs, n_pairs");
      for (int l = 0; l < h->n_leaves; ++l)
        if (obs->pair_begin[l] < 0 || obs->pair_begin[l + 1] < obs->pair_begin[l] ||
            obs->pair_begin[l + 1] > obs->n_pairs)
          return fail(h, RMP2_ERR_INVALID_ARGUMENT, "pair_begin must be non-decreasing within [0, n_pairs]");
      if (!h->pair_begin_valid || std::memcmp(h->h_pair_begin, obs->pair_begin, sizeof(h->h_pair_begin)) != 0) {
        // the ranges change only when the caller's pair layout changes; refresh the device copy then
        std::memcpy(h->h_pair_begin, obs->pair_begin, sizeof(h->h_pair_begin));
        HIP_TRY(h, hipMemcpyAsync(h->d_pair_begin, h->h_pair_begin, sizeof(h->h_pair_begin), hipMemcpyHostToDevice, s));
        h->pair_begin_valid = true;
      }
    } else if (o.mode == RMP2_OBS_SHARED_SPHERES || o.mode == RMP2_OBS_RAGGED_SPHERES) {
      if (obs->n_spheres < 0 || (obs->n_spheres > 0 && !obs->spheres))
        return fail(h, RMP2_ERR_INVALID_ARGUMENT, "sphere table missing");
      if (obs->primitive != RMP2_PRIM_SPHERE && obs->primitive != RMP2_PRIM_CAPSULE && obs->primitive != RMP2_PRIM_CYLINDER)
        return fail(h, RMP2_ERR_INVALID_ARGUMENT, "unknown obstacle primitive");
      if (obs->primitive == RMP2_PRIM_CYLINDER && (obs->link_capsules || h->has_point))   // (plain steps over a shared table never get here: stage_link_geometry)
        return fail(h, RMP2_ERR_UNSUPPORTED, "cylinder tables with link geometry in a rollout / over ragged lists / for attached-point leaves: the "
                                             "nearest points of a segment and a cylinder are an iteration -- rmp2_closest_points_links + EXPLICIT_PAIRS");
      if (o.mode == RMP2_OBS_RAGGED_SPHERES && (!obs->csr_offset || (!obs->csr_index && obs->n_spheres > 0)))
        return fail(h, RMP2_ERR_INVALID_ARGUMENT, "RAGGED_SPHERES needs csr_offset / csr_index");
    } else {
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, "unknown obstacle mode");
    }
    o.n_spheres = obs->n_spheres;
    o.n_pairs = obs->n_pairs;
    o.capsule = (o.mode != RMP2_OBS_EXPLICIT_PAIRS && obs->primitive != RMP2_PRIM_SPHERE) ? 1 : 0;   // (8-float records)
    o.cylinder = (o.mode != RMP2_OBS_EXPLICIT_PAIRS && obs->primitive == RMP2_PRIM_CYLINDER) ? 1 : 0;
    o.spheres = obs->spheres;
    o.p_link = obs->p_link;
    o.p_obs = obs->p_obs;
    o.csr_offset = obs->csr_offset;
    o.csr_index = obs->csr_index;
    o.dist = obs->dist;
    o.pair_begin = h->d_pair_begin;
    if (obs->link_capsules) {
      // link geometry inside the step (quad mapping, attached-record builds): see include/rmp2.h rmp2_obstacles
      // (ragged lists since round 4: as membership masks over tables of <= 64 primitives, by a list walk otherwise; sets with
      // attached-point leaves keep the shared table -- their pairs are not culled per list)
      const bool ragged_ok = o.mode == RMP2_OBS_RAGGED_SPHERES && !h->has_point;
      if ((o.mode != RMP2_OBS_SHARED_SPHERES && !ragged_ok) || obs->n_spheres > kLdsSpheres)
        return fail(h, RMP2_ERR_UNSUPPORTED, "link_capsules: SHARED_SPHERES / RAGGED_SPHERES tables of at most 256 primitives "
                                             "(otherwise: rmp2_closest_points_links + EXPLICIT_PAIRS)");
      if (!fused_link_geometry_fits(h, obs))
        return fail(h, RMP2_ERR_UNSUPPORTED, "link_capsules: robots with at most 9 dofs; solve = pinv only where the quad mapping "
                                             "certifies or computes it (otherwise: rmp2_closest_points_links + EXPLICIT_PAIRS)");
      o.link_caps = obs->link_capsules;
    }
  }
  oa = OutArgs{out->qdd, out->status, out->M, out->f};
  return RMP2_OK;
}

// handles whose plain step is two kernels with the combined systems in between (dispatch_solve)
static bool needs_system_buffer(const rmp2_handle* h) {
  return (h->strict || h->likely_singular) && !quad_certifies_strict(h) && h->n_template == 9;
}

// Link geometry over RAGGED lists beyond the fused limits (stage_link_geometry): the closest-point stage has written, per robot, the pairs of
// every distance leaf with EVERY primitive of the table (leaf i owns pairs [i K, (i + 1) K)); this kernel lays out what the robot's
// list asks for -- one pair per LIST ENTRY, so that an index a list repeats counts twice, as the fused list walk counts it -- at L
// slots per leaf, L = the longest list of the fleet.  Slots beyond a robot's list (and entries outside the table) hold a filler
// pair: the leaf's first control point and an obstacle point 1e9 m from it -- beyond any avoidance radius, metric exactly 0,
// every other term finite (what tests/test_gpu_capsules.py's oracle pairs use, a kilometre away).
constexpr float kFillerDistance = 1.0e9f;
__global__ void __launch_bounds__(kWave) rmp2_gather_list_pairs_kernel(const float* __restrict__ pl_all, const float* __restrict__ po_all,
                                                                      const int32_t* __restrict__ csr_offset,
                                                                      const int32_t* __restrict__ csr_index, float* __restrict__ pl_out,
                                                                      float* __restrict__ po_out, int n_dist, int K, int L, int R) {
  const int r = blockIdx.x;
  if (r >= R) return;
  const int off = csr_offset[r], len = csr_offset[r + 1] - off;
  const size_t in0 = (size_t)r * n_dist * K, out0 = (size_t)r * n_dist * L;
  for (int t = threadIdx.x; t < n_dist * L; t += kWave) {
    const int i = t / L, e = t - i * L;
    const int k = e < len ? csr_index[off + e] : -1;
    const bool member = k >= 0 && k < K;
    const size_t src = (in0 + (size_t)i * K + (member ? k : 0)) * 3, dst = (out0 + t) * 3;
    const float a0 = pl_all[src], a1 = pl_all[src + 1], a2 = pl_all[src + 2];
    pl_out[dst] = a0, pl_out[dst + 1] = a1, pl_out[dst + 2] = a2;
    po_out[dst] = member ? po_all[src] : a0 + kFillerDistance;
    po_out[dst + 1] = member ? po_all[src + 1] : a1;
    po_out[dst + 2] = member ? po_all[src + 2] : a2;
  }
}

static int grow_system_buffer(rmp2_handle* h, int32_t R) {
  h->system_robots = 0;
  if (int rc = realloc_device(h, &h->d_system, sizeof(double) * (size_t)R * h->n_dof * (h->n_dof + 1))) return rc;
  h->system_robots = (size_t)R;
  return RMP2_OK;
}

int rmp2_reserve(rmp2_handle* h, int32_t R) {
  if (!h || R < 0) return RMP2_ERR_INVALID_ARGUMENT;
  if (int rc = use_device(h)) return rc;
  if (needs_system_buffer(h) && (size_t)R > h->system_robots) return grow_system_buffer(h, R);
  return RMP2_OK;
}

// What the stage kernels read of a shared primitive table (NULL: no table, all zero).
static ObsArgs shared_table_args(const rmp2_obstacles* table) {
  ObsArgs o;
  std::memset(&o, 0, sizeof(o));
  if (!table) return o;
  o.mode = table->mode;
  o.n_spheres = table->n_spheres;
  o.capsule = table->primitive != RMP2_PRIM_SPHERE ? 1 : 0;   // (8-float records)
  o.cylinder = table->primitive == RMP2_PRIM_CYLINDER ? 1 : 0;
  o.spheres = table->spheres;
  return o;
}

// Launch of rmp2_self_stage_kernel: `table` = a SHARED_SPHERES table whose pairs come first in each distance leaf's range, or
// NULL (self pairs only).  P = pairs per robot of the layout.
static int launch_self_stage(rmp2_handle* h, const float* q, const rmp2_obstacles* table, float* p_link, float* p_obs, float* dist,
                             int P, int32_t R, hipStream_t s) {
  const ObsArgs o = shared_table_args(table);
  const int n_dist = (int)h->distance_leaves.size();
  const bool with_table = table != nullptr;
  const int W = self_lds_records(with_table ? n_dist : 0, (int)h->pair_leaves.size(), h->self_n_b);
  // robots per wave: kClosestRobots (64 per wave measured slower for config 3 at 65 536 robots: 105 against 72 us for the self
  // stage alone -- a quarter of the waves, each walking phase 2 for four times the robots)
  const int nr = kClosestRobots;
  const size_t lds_bytes = sizeof(float4) * (size_t)W * nr;
  const int blocks = (R + nr - 1) / nr;
  const SelfProg* sp = static_cast<const SelfProg*>(h->d_self);
  const float* lc = with_table ? table->link_capsules : nullptr;
#define RMP2_SELF_STAGE_(OBS_, LINK_, CAPS_)                                                                                   \
  hipLaunchKernelGGL((rmp2_self_stage_kernel<2, OBS_, LINK_, CAPS_>), dim3(blocks), dim3(kWave), lds_bytes, s, h->d_prog,      \
                     h->d_prog_full, sp, q, o, lc, p_link, p_obs, dist, P, (int)R, nr)
  if (!with_table) RMP2_SELF_STAGE_(false, false, false);
  else if (lc && o.capsule) RMP2_SELF_STAGE_(true, true, true);
  else if (lc) RMP2_SELF_STAGE_(true, true, false);
  else if (o.capsule) RMP2_SELF_STAGE_(true, false, true);
  else RMP2_SELF_STAGE_(true, false, false);
#undef RMP2_SELF_STAGE_
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

// Launch of rmp2_hull_stage_kernel over a SHARED_SPHERES sphere / capsule table (K > 0): pair leaf o owns pairs [o K, (o + 1) K).
// The hulls are the handle's HullProg: its link hulls, or with hull self pairs the pair leaves' hulls of that list (whose HullProg
// places each leaf's obstacle pairs in front of its self pairs).
static int launch_hull_stage(rmp2_handle* h, const float* q, const rmp2_obstacles* table, float* p_link, float* p_obs, float* dist,
                             int32_t R, hipStream_t s) {
  const int L = (int)h->pair_leaves.size(), K = table->n_spheres;
  const size_t lds_bytes = sizeof(float4) * 3 * (size_t)L * kHullRobots;
  const int blocks = (R + kHullRobots - 1) / kHullRobots;
  const HullProg* hp = static_cast<const HullProg*>(h->d_hull);
  const float4* tab = reinterpret_cast<const float4*>(table->spheres);
#define RMP2_HULL_STAGE_(CAPS_)                                                                                              \
  hipLaunchKernelGGL((rmp2_hull_stage_kernel<S, CAPS_>), dim3(blocks), dim3(kWave), lds_bytes, s, h->d_prog, hp,           \
                     h->d_hull_verts, h->d_hull_planes, q, tab, K, p_link, p_obs, dist, (int)R)
  const bool caps = table->primitive == RMP2_PRIM_CAPSULE;
  with_slots(h->n_slots, [&](auto S) {
    if (caps) RMP2_HULL_STAGE_(true);
    else RMP2_HULL_STAGE_(false);
  });
#undef RMP2_HULL_STAGE_
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

// Launch of the hull self-pair stage: with `table` (a SHARED_SPHERES sphere / capsule table, K > 0) rmp2_hull_stage_kernel first
// forms the K obstacle pairs of each leaf on the leaves' hulls, then rmp2_self_hull_stage_kernel the self pairs behind them;
// without, the self pairs alone.  P = pairs per robot of the layout.
static int launch_self_hull_stage(rmp2_handle* h, const float* q, const rmp2_obstacles* table, float* p_link, float* p_obs, float* dist,
                                  int P, int32_t R, hipStream_t s) {
  const int K = table ? table->n_spheres : 0;
  if (K > 0)
    if (int rc = launch_hull_stage(h, q, table, p_link, p_obs, dist, R, s)) return rc;
  const int slots = h->shull_slots;
  int nr = kSelfHullRobots;
  while (nr > 1 && sizeof(float) * 12 * (size_t)slots * nr > 64 * 1024) nr /= 2;
  const size_t lds_bytes = sizeof(float) * 12 * (size_t)(slots > 0 ? slots : 1) * nr;
  const int blocks = (R + nr - 1) / nr;
  const SelfHullProg* sp = static_cast<const SelfHullProg*>(h->d_shull);
  with_slots(h->n_slots_full, [&](auto S) {   // (the kernel walks the unpruned program: its save slots, not the step's)
    hipLaunchKernelGGL((rmp2_self_hull_stage_kernel<S>), dim3(blocks), dim3(kWave), lds_bytes, s, h->d_prog_full, sp,
                       h->d_hull_verts, h->d_hull_planes, q, p_link, p_obs, dist, P, K, (int)R, nr);
  });
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

// Grows the handle's stage buffer (rmp2_host.h d_stage) to `need` floats for the stage of `what` (a step of R robots).  Refused inside
// a stream capture and beyond free device memory.
static int grow_stage_buffer(rmp2_handle* h, size_t need, int32_t R, hipStream_t s, const std::string& what) {
  if (need <= h->stage_floats) return RMP2_OK;
  if (capturing(s))
    return fail(h, RMP2_ERR_UNSUPPORTED, what + " as stage + explicit-pair step: the handle's pair buffer must grow -- step once "
                                                "outside the capture first");
  if (int rc = use_device(h)) return rc;
  if (h->d_stage) HIP_TRY(h, hipFree(h->d_stage));   // (synchronises the device: no launch still reads the old buffer)
  h->d_stage = nullptr, h->stage_floats = 0;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
  if (sizeof(float) * need > free_b)
    return fail(h, RMP2_ERR_UNSUPPORTED, what + ": the stage's pair buffer needs " + std::to_string(sizeof(float) * need) + " bytes (" +
                                             std::to_string(sizeof(float) * need / (size_t)R) + " per robot), " + std::to_string(free_b) +
                                             " bytes of device memory are free -- step a smaller fleet");
  HIP_TRY(h, hipMalloc(&h->d_stage, sizeof(float) * need));
  h->stage_floats = need;
  return RMP2_OK;
}

// The stage buffer as p_link | p_obs [R][P][3] (+ dist [R][P] with attached-point leaves) -- 24 P (+ 4 P) bytes per robot
// (include/rmp2.h) --, grown for the stage of `what`.
static int stage_arrays(rmp2_handle* h, size_t P, int32_t R, hipStream_t s, const char* what, float*& pl, float*& po, float*& dd) {
  const size_t arr = (size_t)R * P * 3;
  if (int rc = grow_stage_buffer(h, 2 * arr + (h->has_point ? (size_t)R * P : 0), R, s, what)) return rc;
  if (int rc = use_device(h)) return rc;
  pl = h->d_stage, po = pl + arr, dd = h->has_point ? po + arr : nullptr;
  return RMP2_OK;
}

// The staged step of a handle with self collision (include/rmp2.h): validates the obstacle input, forms every pair leaf's range
// [K obstacle pairs | S_l self pairs] in the handle's stage buffer, described as EXPLICIT_PAIRS in `staged` and put in *obs.
static int stage_self(rmp2_handle* h, const float* q, const rmp2_obstacles*& obs, int32_t R, hipStream_t s, rmp2_obstacles& staged) {
  const int mode = obs ? obs->mode : RMP2_OBS_NONE;
  if (mode == RMP2_OBS_EXPLICIT_PAIRS)
    return fail(h, RMP2_ERR_UNSUPPORTED, "self collision with caller-supplied EXPLICIT_PAIRS: the self pairs would have to be merged "
                                         "into the caller's ranges -- append rmp2_self_pairs' output to them and step a handle without "
                                         "self collision");
  if (mode == RMP2_OBS_RAGGED_SPHERES)
    return fail(h, RMP2_ERR_UNSUPPORTED, "self collision over RAGGED_SPHERES lists: not supported (shared tables only)");
  if (mode != RMP2_OBS_NONE && mode != RMP2_OBS_SHARED_SPHERES) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "unknown obstacle mode");
  if (!q) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "q, qd and out->qdd are required");
  const bool with_table = mode == RMP2_OBS_SHARED_SPHERES && obs->n_spheres != 0;
  if (with_table) {
    if (obs->n_spheres < 0 || !obs->spheres) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "sphere table missing");
    if (obs->primitive == RMP2_PRIM_CYLINDER)
      return fail(h, RMP2_ERR_UNSUPPORTED, "self collision with a CYLINDER table: not supported (sphere or capsule records)");
    if (obs->primitive != RMP2_PRIM_SPHERE && obs->primitive != RMP2_PRIM_CAPSULE)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, "unknown obstacle primitive");
    if (h->has_point)
      return fail(h, RMP2_ERR_UNSUPPORTED, "self collision with an obstacle table on a set with attached-point leaves: not supported "
                                           "(obstacle input NONE, or a set of distance leaves)");
  }
  if (h->self_hulls && mode == RMP2_OBS_SHARED_SPHERES && obs->link_capsules)
    return fail(h, RMP2_ERR_UNSUPPORTED, "link_capsules given together with hull self pairs: the obstacle pairs are formed on the same "
                                         "hulls (turn the hulls off with rmp2_set_self_collision(h, 0, ...) to step on capsules)");
  if (h->self_hulls && with_table && h->shull_leaf_empty)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "hull self pairs with an obstacle table: every distance leaf needs a hull (an entry is empty)");
  const int K = with_table ? obs->n_spheres : 0;
  auto pairs_of = [&](int o) { return (size_t)(h->pair_leaf_point[o] ? 0 : K) + (size_t)h->self_counts[o]; };
  size_t P = 0;
  for (int o = 0; o < (int)h->pair_leaves.size(); ++o) P += pairs_of(o);
  if (P > (size_t)INT32_MAX / 4) return fail(h, RMP2_ERR_UNSUPPORTED, "self collision: too many pairs per robot");
  float *pl, *po, *dd;
  if (int rc = stage_arrays(h, P, R, s, "self collision", pl, po, dd)) return rc;
  if (h->self_hulls) {
    if (int rc = launch_self_hull_stage(h, q, with_table ? obs : nullptr, pl, po, dd, (int)P, R, s)) return rc;
  } else if (int rc = launch_self_stage(h, q, with_table ? obs : nullptr, pl, po, dd, (int)P, R, s)) {
    return rc;
  }
  explicit_pairs(h->pair_leaves, pairs_of, pl, po, dd, staged);
  obs = &staged;
  return RMP2_OK;
}

// The obstacle table of a hull stage (rmp2_closest_points_hulls and the staged step): a SHARED_SPHERES table of sphere or capsule
// records without link_capsules.
static int check_hull_table(rmp2_handle* h, const rmp2_obstacles* t) {
  if (t->mode == RMP2_OBS_EXPLICIT_PAIRS)
    return fail(h, RMP2_ERR_UNSUPPORTED, "link hulls with caller-supplied EXPLICIT_PAIRS: the hulls form the pairs from a table -- "
                                         "step a handle without hulls on the arrays of rmp2_closest_points_hulls");
  if (t->mode == RMP2_OBS_RAGGED_SPHERES)
    return fail(h, RMP2_ERR_UNSUPPORTED, "link hulls over RAGGED_SPHERES lists: not supported (shared tables only)");
  if (t->mode != RMP2_OBS_SHARED_SPHERES) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "link hulls need a SHARED_SPHERES table");
  if (t->n_spheres < 0 || (t->n_spheres > 0 && !t->spheres)) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "sphere table missing");
  if (t->primitive == RMP2_PRIM_CYLINDER)
    return fail(h, RMP2_ERR_UNSUPPORTED, "link hulls with a CYLINDER table: not supported (sphere or capsule records)");
  if (t->primitive != RMP2_PRIM_SPHERE && t->primitive != RMP2_PRIM_CAPSULE)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "unknown obstacle primitive");
  if (t->link_capsules)
    return fail(h, RMP2_ERR_UNSUPPORTED, "link_capsules given together with link hulls: one link geometry per handle (turn the hulls "
                                         "off with rmp2_set_link_hulls(h, 0, ...) to step on capsules)");
  return RMP2_OK;
}

// The staged step of a handle with link hulls (include/rmp2.h): the hull stage into the handle's stage buffer, described as
// EXPLICIT_PAIRS in `staged` and put in *obs; obstacle input NONE or an empty table: nothing to stage (*obs unchanged).
static int stage_hulls(rmp2_handle* h, const float* q, const rmp2_obstacles*& obs, int32_t R, hipStream_t s, rmp2_obstacles& staged) {
  if (!obs || obs->mode == RMP2_OBS_NONE) return RMP2_OK;
  if (int rc = check_hull_table(h, obs)) return rc;
  if (obs->n_spheres == 0) return RMP2_OK;
  if (!q) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "q, qd and out->qdd are required");
  const int K = obs->n_spheres;
  const size_t P = h->pair_leaves.size() * (size_t)K;
  if (P > (size_t)INT32_MAX / 4) return fail(h, RMP2_ERR_UNSUPPORTED, "link hulls: too many pairs per robot");
  float *pl, *po, *dd;
  if (int rc = stage_arrays(h, P, R, s, "link hulls", pl, po, dd)) return rc;
  if (int rc = launch_hull_stage(h, q, obs, pl, po, dd, R, s)) return rc;
  explicit_pairs(h->pair_leaves, [K](int) { return K; }, pl, po, dd, staged);
  obs = &staged;
  return RMP2_OK;
}

// Link geometry of the distance leaves beyond what the fused forms take (include/rmp2.h rmp2_obstacles.link_capsules: robots with more
// than nine dofs, solve = pinv where the quad mapping does not certify it, sets without an inertia leaf, tables beyond 256 primitives,
// CYLINDER tables -- whose segment-cylinder closed form is an iteration): the step runs as the reference's own data flow instead
// (simulation.py:462-484 -> data_management.py:22-37 -> taskmap.py:115-138) -- the closest-point stage into the handle's stage buffer,
// then the explicit-pair step on it.  Same pairs, same semantics; two launches.  (Plain control steps of distance-leaf sets; rollouts
// keep the fused forms' limits.)
static bool stages_link_geometry(const rmp2_handle* h, const rmp2_obstacles* obs, const RolloutArgs& ro) {
  return obs && obs->link_capsules && (obs->mode == RMP2_OBS_SHARED_SPHERES || obs->mode == RMP2_OBS_RAGGED_SPHERES) && !h->has_point &&
         ro.n_iters == 1 && ro.substeps == 0 && obs->n_spheres > 0 && obs->spheres && !h->distance_leaves.empty() &&
         !fused_link_geometry_fits(h, obs);
}

// The staged link-geometry step (stages_link_geometry): rmp2_closest_points_links pairs every distance leaf with every primitive
// (leaf i owns pairs [i K, (i + 1) K)).  RAGGED lists take one more launch: rmp2_gather_list_pairs_kernel lays out one pair per list
// entry at L = the fleet's longest list slots per leaf -- L is read back from csr_offset, so this form synchronises the stream and is
// refused inside a stream capture.  The result is described as EXPLICIT_PAIRS in `staged` and put in *obs.
static int stage_link_geometry(rmp2_handle* h, const float* q, const rmp2_obstacles*& obs, int32_t R, hipStream_t s,
                               rmp2_obstacles& staged) {
  const bool ragged_lists = obs->mode == RMP2_OBS_RAGGED_SPHERES;
  const int K = obs->n_spheres;
  const size_t n_dist = h->distance_leaves.size();
  const size_t P_all = n_dist * (size_t)K;   // the stage's pairs per robot: every leaf with every primitive
  int L = 0;
  if (ragged_lists) {
    if (!obs->csr_offset || !obs->csr_index) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "RAGGED_SPHERES needs csr_offset / csr_index");
    if (capturing(s))
      return fail(h, RMP2_ERR_UNSUPPORTED, "link geometry over ragged lists as stage + explicit-pair step reads the list lengths back: "
                                           "not inside a stream capture");
    if (int rc = use_device(h)) return rc;
    HIP_TRY(h, hipStreamSynchronize(s));   // (the lists may have been written on this stream)
    std::vector<int32_t> offs((size_t)R + 1);
    HIP_TRY(h, hipMemcpy(offs.data(), obs->csr_offset, sizeof(int32_t) * offs.size(), hipMemcpyDeviceToHost));
    size_t longest = 0;
    for (int32_t r = 0; r < R; ++r) {
      if (offs[r + 1] < offs[r]) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "csr_offset must not decrease");
      longest = std::max(longest, (size_t)(offs[r + 1] - offs[r]));
    }
    longest = std::max<size_t>(longest, 1);   // (every list empty: one filler pair per leaf)
    if (n_dist * longest > (size_t)INT32_MAX / 4) return fail(h, RMP2_ERR_UNSUPPORTED, "ragged lists too long for the explicit-pair step");
    L = (int)longest;
  }
  // buffer: p_link [all | out] then p_obs [all | out], all = [R][P_all][3], out = [R][n_dist L][3] over ragged lists
  const size_t all = (size_t)R * P_all * 3;
  const size_t arr = all + (ragged_lists ? (size_t)R * n_dist * L * 3 : 0);
  if (int rc = grow_stage_buffer(h, 2 * arr, R, s, "link geometry")) return rc;
  float* const pl = h->d_stage;
  float* const po = pl + arr;
  rmp2_obstacles table = *obs;
  table.link_capsules = nullptr;
  table.mode = RMP2_OBS_SHARED_SPHERES;   // (the stage pairs every leaf with every primitive; a ragged fleet's lists pick below)
  table.csr_offset = table.csr_index = nullptr;
  if (int rc = rmp2_closest_points_links(h, q, &table, obs->link_capsules, pl, po, R, s)) return rc;
  if (ragged_lists) {
    hipLaunchKernelGGL(rmp2_gather_list_pairs_kernel, dim3(R), dim3(kWave), 0, s, pl, po, obs->csr_offset, obs->csr_index, pl + all,
                       po + all, (int)n_dist, K, L, (int)R);
    HIP_TRY(h, hipGetLastError());
    // leaf ranges at L slots per distance leaf (the stage's were K per leaf; prepare_step uploads the new ones -- after the stage's
    // own upload on the same stream, each from pageable memory, i.e. read before the call returns)
    explicit_pairs(h->distance_leaves, [L](int) { return L; }, pl + all, po + all, nullptr, staged);
  } else {
    explicit_pairs(h->distance_leaves, [K](int) { return K; }, pl, po, nullptr, staged);   // (as the stage laid the pairs out)
  }
  obs = &staged;
  return RMP2_OK;
}

// A control step: at most one stage -- chosen by the handle's state and the obstacle input -- writes the pairs of the step into the
// handle's stage buffer, then the step itself runs.
static int step_impl(rmp2_handle* h, const float* q, const float* qd, const float* goal, int32_t goal_stride,
                     const rmp2_obstacles* obs, const rmp2_outputs* out, const RolloutArgs& ro, int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (R < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "R < 0");
  if (R == 0) return RMP2_OK;  // empty fleet: nothing to do (pointers may be null)
  hipStream_t s = (hipStream_t)stream;
  // (link hulls and self collision exclude each other; after either stage the input is EXPLICIT_PAIRS, never a link-geometry table)
  rmp2_obstacles staged;
  int rc = RMP2_OK;
  if (h->hull_n > 0) rc = stage_hulls(h, q, obs, R, s, staged);
  else if (h->self_n_pairs > 0) rc = stage_self(h, q, obs, R, s, staged);
  else if (stages_link_geometry(h, obs, ro)) rc = stage_link_geometry(h, q, obs, R, s, staged);
  if (rc) return rc;
  ObsArgs o;
  OutArgs oa;
  if ((rc = prepare_step(h, q, qd, goal, goal_stride, obs, out, ro, R, stream, o, oa))) return rc;
  if (needs_system_buffer(h) && (size_t)R > h->system_robots) {
    // the combined systems between the two kernels of the strict step (dispatch_solve): 8 n (n + 1) bytes per robot, owned by
    // the handle, grown to the largest fleet stepped.  Not during a stream capture (an allocation there is illegal):
    // rmp2_reserve(h, R) first.
    if (capturing(s))
      return fail(h, RMP2_ERR_UNSUPPORTED, "this handle's two-kernel step needs its system buffer grown: call rmp2_reserve(h, R) "
                                           "before capturing the stream");
    if ((rc = grow_system_buffer(h, R))) return rc;
  }
  if (h->n_template == 2)
    rc = dispatch_solve<2>(h, q, qd, goal, goal_stride, o, oa, ro, R, s);
  else if (h->n_template == 9)
    rc = dispatch_solve<9>(h, q, qd, goal, goal_stride, o, oa, ro, R, s);
  else  // 10 .. 16 dofs: hex mapping at every fleet size
    rc = launch_hex_n16(h, q, qd, goal, goal_stride, o, oa, ro, R, s) ? RMP2_OK : RMP2_ERR_UNSUPPORTED;
  if (rc != RMP2_OK) return fail(h, rc, "no kernel instantiation for this robot");
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

// The staged handles (self collision, link hulls) step through rmp2_step only: refused by `entry`, `why` says what to do instead.
static int refuse_staged(rmp2_handle* h, const char* entry, const char* why) {
  const char* what = h->self_n_pairs > 0 ? "self collision" : (h->hull_n > 0 ? "link hulls" : nullptr);
  if (!what) return RMP2_OK;
  return fail(h, RMP2_ERR_UNSUPPORTED, std::string(what) + ": not in " + entry + " (" + why + ")");
}

int rmp2_step(rmp2_handle* h, const float* q, const float* qd, const float* goal, int32_t goal_stride,
              const rmp2_obstacles* obs, const rmp2_outputs* out, int32_t R, void* stream) {
  const RolloutArgs ro{1, 0, 0.f, nullptr, nullptr, 0};
  return step_impl(h, q, qd, goal, goal_stride, obs, out, ro, R, stream);
}

// ---- native obstacle exchange (include/rmp2.h): RCCL all-gather of the sphere table + step, one call per control step ----
// RCCL is bound at run time (dlopen of the library the caller names -- the copy the process already uses, e.g. PyTorch's --
// so that librmp2_hip.so itself has no link-time dependency on it and a fleet without a distributed table never loads it).
namespace {
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, rmp2_rccl_uid, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;      // optional: what the communicator itself says about its size and this rank
  int (*CommUserRank)(void*, int*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
constexpr int kNcclFloat = 7;  // ncclFloat32 (rccl.h ncclDataType_t)

int load_rccl(const char* path, RcclApi& api, std::string& err) {
  if (!path || !*path) return err = "path of the RCCL library is required", RMP2_ERR_INVALID_ARGUMENT;
  api.lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!api.lib) return err = std::string("dlopen(") + path + "): " + dlerror(), RMP2_ERR_HIP;
  api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.lib, "ncclGetUniqueId"));
  api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.lib, "ncclCommInitRank"));
  api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(api.lib, "ncclAllGather"));
  api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.lib, "ncclCommDestroy"));
  api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.lib, "ncclGetErrorString"));
  api.CommCount = reinterpret_cast<decltype(api.CommCount)>(dlsym(api.lib, "ncclCommCount"));
  api.CommUserRank = reinterpret_cast<decltype(api.CommUserRank)>(dlsym(api.lib, "ncclCommUserRank"));
  if (!api.GetUniqueId || !api.CommInitRank || !api.AllGather || !api.CommDestroy)
    return err = std::string(path) + " does not export the RCCL entry points", RMP2_ERR_HIP;
  return RMP2_OK;
}
}  // namespace

struct rmp2_exchange {
  static constexpr int kBuf = 3;                   // table buffers, all in rotation at either depth (see rmp2_exchange_set_depth)
  RcclApi api;
  void* comm = nullptr;
  int device = 0, rank = 0, world = 1, per_rank = 0;
  int comm_count = 0, comm_rank = -1;              // ncclCommCount / ncclCommUserRank of the communicator that formed (0 / -1: not exported)
  int depth = 1;                                   // gathers that may be outstanding minus one ... see rmp2_exchange_set_depth
  int nbuf = kBuf;                                 // table buffers in rotation: all kBuf; depth + 1 with RMP2_EXCHANGE_BUFFERS=2 (A/B)
  bool all_buffers = true;
  float* table[kBuf] = {nullptr, nullptr, nullptr};    // [world * per_rank][4]
  hipStream_t side = nullptr;                      // the gathers' stream
  hipEvent_t ready[kBuf] = {nullptr, nullptr, nullptr};        // gather into table b complete
  hipEvent_t reader_done[kBuf] = {nullptr, nullptr, nullptr};  // last kernel that read table b complete (the launch's own stop event)
  hipEvent_t produced = nullptr;                   // "everything enqueued on the caller's stream so far"
  bool reader_valid[kBuf] = {false, false, false};
  int pending[kBuf] = {0, 0, 0}, n_pending = 0, next = 0;
  bool peer_wait = false;  // keep the GPU-side wait at world 1 too (the single-GPU emulation of an N-rank run: rmp2_exchange_set_peer_wait)
  int throttle_us = 500;  // bound of the host throttle in rmp2_exchange_step (0: free-running; RMP2_EXCHANGE_THROTTLE_US)
  std::string error;
};

int rmp2_exchange_unique_id(const char* rccl_library, rmp2_rccl_uid* uid) {
  if (!uid) return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "null argument");
  RcclApi api;
  std::string err;
  if (int rc = load_rccl(rccl_library, api, err)) return fail(nullptr, rc, err);
  const int r = api.GetUniqueId(uid);
  return r == 0 ? RMP2_OK : fail(nullptr, RMP2_ERR_HIP, std::string("ncclGetUniqueId: ") + (api.GetErrorString ? api.GetErrorString(r) : "?"));
}

int rmp2_exchange_create(const char* rccl_library, const rmp2_rccl_uid* uid, int rank, int nranks, int device,
                         int spheres_per_rank, rmp2_exchange** out) {
  if (!out || !uid || nranks < 1 || rank < 0 || rank >= nranks || spheres_per_rank < 1)
    return fail(nullptr, RMP2_ERR_INVALID_ARGUMENT, "rmp2_exchange_create: bad arguments");
  *out = nullptr;
  rmp2_exchange* x = new (std::nothrow) rmp2_exchange();
  if (!x) return fail(nullptr, RMP2_ERR_HIP, "out of host memory");
  x->device = device, x->rank = rank, x->world = nranks, x->per_rank = spheres_per_rank;
  if (const char* te = std::getenv("RMP2_EXCHANGE_THROTTLE_US")) x->throttle_us = std::max(0, std::atoi(te));
  if (const char* tb = std::getenv("RMP2_EXCHANGE_BUFFERS")) x->all_buffers = std::atoi(tb) >= rmp2_exchange::kBuf;
  x->nbuf = x->all_buffers ? rmp2_exchange::kBuf : x->depth + 1;
  std::string err;
  int rc = load_rccl(rccl_library, x->api, err);
  hipError_t e = hipSuccess;
  if (rc == RMP2_OK) {
    e = hipSetDevice(device);
    // ready[]: a default event (system-scope release) when peers write the table over xGMI, a device-scope one for one rank;
    // reader_done[] / produced order work of THIS GPU only (rmp2_fence_* rules)
    const unsigned ready_flags = hipEventDisableTiming | (nranks == 1 ? hipEventDisableSystemFence : 0u);
    const unsigned local_flags = hipEventDisableTiming | hipEventDisableSystemFence;
    for (int b = 0; b < rmp2_exchange::kBuf && e == hipSuccess; ++b) {
      e = hipMalloc(&x->table[b], sizeof(float) * 4 * nranks * spheres_per_rank);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&x->ready[b], ready_flags);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&x->reader_done[b], local_flags);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&x->produced, local_flags);
    if (e == hipSuccess) {
      // highest priority: at the boundary between two step kernels the gather's few workgroups are dispatched BEFORE the next
      // step's 4 096 (which fill every SIMD and all of LDS; behind them the gather would only run at that step's tail)
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
      e = hipStreamCreateWithPriority(&x->side, hipStreamNonBlocking, hi);
    }
    if (e != hipSuccess) rc = RMP2_ERR_HIP, err = std::string("rmp2_exchange_create: ") + hipGetErrorString(e);
  }
  if (rc == RMP2_OK) {
    const int r = x->api.CommInitRank(&x->comm, nranks, *uid, rank);
    if (r != 0) rc = RMP2_ERR_HIP, err = std::string("ncclCommInitRank: ") + (x->api.GetErrorString ? x->api.GetErrorString(r) : "?");
  }
  if (rc == RMP2_OK && x->api.CommCount && x->api.CommUserRank) {
    // the communicator's own word on its size and this rank: the table is laid out for `nranks` slices, so one that formed with
    // another size (or put this rank elsewhere) would gather into the wrong offsets -- refuse it here, not in the first step
    if (x->api.CommCount(x->comm, &x->comm_count) != 0 || x->api.CommUserRank(x->comm, &x->comm_rank) != 0)
      x->comm_count = 0, x->comm_rank = -1;
    else if (x->comm_count != nranks || x->comm_rank != rank)
      rc = RMP2_ERR_HIP, err = "the communicator formed with " + std::to_string(x->comm_count) + " rank(s), this one as rank " +
                               std::to_string(x->comm_rank) + "; asked for rank " + std::to_string(rank) + " of " + std::to_string(nranks);
  }
  if (rc != RMP2_OK) {
    rmp2_exchange_destroy(x);
    return fail(nullptr, rc, err);
  }
  *out = x;
  return RMP2_OK;
}

int rmp2_exchange_destroy(rmp2_exchange* x) {
  if (!x) return RMP2_OK;
  (void)hipSetDevice(x->device);
  if (x->side) (void)hipStreamSynchronize(x->side);
  if (x->comm && x->api.CommDestroy) x->api.CommDestroy(x->comm);
  for (int b = 0; b < rmp2_exchange::kBuf; ++b) {
    if (x->table[b]) (void)hipFree(x->table[b]);
    if (x->ready[b]) (void)hipEventDestroy(x->ready[b]);
    if (x->reader_done[b]) (void)hipEventDestroy(x->reader_done[b]);
  }
  if (x->produced) (void)hipEventDestroy(x->produced);
  if (x->side) (void)hipStreamDestroy(x->side);
  delete x;
  return RMP2_OK;
}

int rmp2_exchange_set_peer_wait(rmp2_exchange* x, int32_t on) {
  if (!x) return RMP2_ERR_INVALID_ARGUMENT;
  x->peer_wait = on != 0;
  return RMP2_OK;
}

int rmp2_exchange_set_depth(rmp2_exchange* x, int32_t depth) {
  if (!x || depth < 1 || depth > rmp2_exchange::kBuf - 1) return RMP2_ERR_INVALID_ARGUMENT;
  if (x->n_pending != 0) return x->error = "set the depth before the first gather is started", RMP2_ERR_INVALID_ARGUMENT;
  x->depth = depth;
  x->nbuf = x->all_buffers ? rmp2_exchange::kBuf : depth + 1;
  x->next = 0;
  return RMP2_OK;
}

int rmp2_exchange_pending(const rmp2_exchange* x) { return x ? x->n_pending : 0; }

const char* rmp2_exchange_last_error(const rmp2_exchange* x) { return x ? x->error.c_str() : g_create_error.c_str(); }

#define XCH_TRY(x, expr)                                                                                   \
  do {                                                                                                     \
    hipError_t e_ = (expr);                                                                                \
    if (e_ != hipSuccess) return (x)->error = std::string(#expr) + ": " + hipGetErrorString(e_), RMP2_ERR_HIP; \
  } while (0)

// Issue the all-gather of `local` ([spheres_per_rank][4], device) into the free table buffer, on the exchange's side
// stream.  It waits for everything enqueued on `stream` so far (the producer of `local`) and for the last kernel that read
// the buffer it overwrites.
int rmp2_exchange_start(rmp2_exchange* x, const float* local, int32_t local_is_ready, void* stream) {
  if (!x || !local) return RMP2_ERR_INVALID_ARGUMENT;
  if (x->n_pending > x->depth)
    return x->error = "too many gathers outstanding (depth + 1): step before starting another", RMP2_ERR_INVALID_ARGUMENT;
  const int b = x->next;
  if (!local_is_ready) {  // order the gather behind the producer of `local` on the caller's stream (an event packet between
    XCH_TRY(x, hipEventRecord(x->produced, static_cast<hipStream_t>(stream)));  // two step kernels: ~4 us of the step)
    XCH_TRY(x, hipStreamWaitEvent(x->side, x->produced, 0));
  }
  if (x->reader_valid[b]) XCH_TRY(x, hipStreamWaitEvent(x->side, x->reader_done[b], 0));
  const int r = x->api.AllGather(local, x->table[b], (size_t)4 * x->per_rank, kNcclFloat, x->comm, x->side);
  if (r != 0) return x->error = std::string("ncclAllGather: ") + (x->api.GetErrorString ? x->api.GetErrorString(r) : "?"), RMP2_ERR_HIP;
  XCH_TRY(x, hipEventRecord(x->ready[b], x->side));
  x->pending[x->n_pending++] = b;
  x->next = (x->next + 1) % x->nbuf;
  return RMP2_OK;
}

// One control step on the oldest outstanding table: `stream` waits for its gather; if `next_local` is given, the gather of
// the NEXT table is issued first (it then takes its few workgroups while the GPU is between two steps, instead of queueing
// behind a kernel that fills every SIMD); then the step kernel is launched with the "table has been read" fence as its own
// completion signal.  `table_out` (optional) receives the device pointer of the table this step reads.
int rmp2_exchange_step(rmp2_exchange* x, rmp2_handle* h, const float* q, const float* qd, const float* goal,
                       int32_t goal_stride, const float* next_local, int32_t next_local_is_ready, const rmp2_outputs* out,
                       int32_t R, void* stream, const float** table_out) {
  if (!x || !h) return RMP2_ERR_INVALID_ARGUMENT;
  if (int rc = refuse_staged(h, "rmp2_exchange_step", "the exchange's step is one launch on the gathered table"))
    return x->error = h->error, rc;
  if (x->n_pending < 1) return x->error = "no gathered table outstanding: rmp2_exchange_start first", RMP2_ERR_INVALID_ARGUMENT;
  const int b = x->pending[0];
  for (int i = 1; i < x->n_pending; ++i) x->pending[i - 1] = x->pending[i];
  --x->n_pending;
  // Host throttle: wait (bounded) until the gather of THIS step's table has completed -- it was issued one call ago and runs
  // as soon as step k - 2 has finished, so the host stays at most ~1.5 steps ahead of the GPU, which is all the launch
  // latency needs.  The point: a stream-wait on an event that has ALREADY completed is dropped by the runtime at enqueue
  // time, while a host that runs many steps ahead turns every one of them into a barrier packet between two step kernels
  // (measured at 65 536 robots: 53.1 us per step free-running, see profiles/r03_exchange_timing.txt).
  bool seen_complete = false;
  if (x->throttle_us > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t qe;
    while ((qe = hipEventQuery(x->ready[b])) == hipErrorNotReady) {
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > x->throttle_us) break;
    }
    seen_complete = qe == hipSuccess;
  }
  // One rank: the gather is a copy on THIS GPU; once the host has seen it complete the step needs no GPU-side wait at all
  // (even a satisfied stream-wait is a barrier packet between two step kernels: 4.7 us of the period,
  // profiles/r03_exchange_timing.txt).  Several ranks: peers wrote the table over xGMI, past this GPU's L2 -- the step
  // keeps the stream-wait on the system-scope event, whose acquire is what makes those writes visible.
  if (!(seen_complete && x->world == 1 && !x->peer_wait))
    XCH_TRY(x, hipStreamWaitEvent(static_cast<hipStream_t>(stream), x->ready[b], 0));
  // The gather of the next table goes out BEFORE the launch (it then takes its few workgroups between two steps) -- unless
  // it would land in the very buffer this step reads (depth + 1 gathers were outstanding, so x->next == b): its only
  // ordering against a reader is reader_done[b], which THIS step has not signalled yet.  Then the step is launched first
  // and the gather is issued behind this launch's completion signal (round-3 advisor finding: a torn table).
  const bool gather_after = next_local && x->next == b;
  if (next_local && !gather_after)
    if (int rc = rmp2_exchange_start(x, next_local, next_local_is_ready, stream)) return rc;
  rmp2_obstacles o;
  std::memset(&o, 0, sizeof(o));
  o.mode = RMP2_OBS_SHARED_SPHERES;
  o.primitive = RMP2_PRIM_SPHERE;
  o.n_spheres = x->world * x->per_rank;
  o.spheres = x->table[b];
  void* const saved = h->step_fence;
  h->step_fence = x->reader_done[b];
  const RolloutArgs ro{1, 0, 0.f, nullptr, nullptr, 0};
  const int rc = step_impl(h, q, qd, goal, goal_stride, &o, out, ro, R, stream);
  h->step_fence = saved;
  if (rc != RMP2_OK) return x->error = h->error, rc;
  x->reader_valid[b] = true;
  if (table_out) *table_out = x->table[b];
  if (gather_after)
    if (int rc2 = rmp2_exchange_start(x, next_local, next_local_is_ready, stream)) return rc2;
  return RMP2_OK;
}

// ncclCommCount of the communicator the exchange joined (queried once, at create); the `nranks` it was created with only where the
// collective library does not export the query.
int rmp2_exchange_nranks(const rmp2_exchange* x) { return !x ? 0 : (x->comm_count > 0 ? x->comm_count : x->world); }

// Two engines, one launch (include/rmp2.h): the fused grid when an instantiation exists for the pair, else two launches.
int rmp2_step_pair(rmp2_handle* ha, const float* qa, const float* qda, const float* goala, int32_t gsa,
                   const rmp2_obstacles* obsa, const rmp2_outputs* outa, int32_t Ra, rmp2_handle* hb, const float* qb,
                   const float* qdb, const float* goalb, int32_t gsb, const rmp2_obstacles* obsb, const rmp2_outputs* outb,
                   int32_t Rb, void* stream) {
  if (!ha || !hb) return RMP2_ERR_INVALID_ARGUMENT;
  for (rmp2_handle* hx : {ha, hb})
    if (int rc = refuse_staged(hx, "rmp2_step_pair", "step the two handles with rmp2_step")) return rc;
  const RolloutArgs ro{1, 0, 0.f, nullptr, nullptr, 0};
  if (Ra > 0 && Rb > 0 && ha->device == hb->device && !ha->step_fence && !hb->step_fence) {
    ObsArgs oa_, ob_;
    OutArgs outa_, outb_;
    if (int rc = prepare_step(ha, qa, qda, goala, gsa, obsa, outa, ro, Ra, stream, oa_, outa_)) return rc;
    if (int rc = prepare_step(hb, qb, qdb, goalb, gsb, obsb, outb, ro, Rb, stream, ob_, outb_)) return rc;
    if (launch_quad_pair(ha, qa, qda, goala, gsa, oa_, outa_, Ra, hb, qb, qdb, goalb, gsb, ob_, outb_, Rb, (hipStream_t)stream)) {
      HIP_TRY(ha, hipGetLastError());
      return RMP2_OK;
    }
  }
  if (int rc = step_impl(ha, qa, qda, goala, gsa, obsa, outa, ro, Ra, stream)) return rc;
  return step_impl(hb, qb, qdb, goalb, gsb, obsb, outb, ro, Rb, stream);
}

int rmp2_rollout(rmp2_handle* h, float* q, float* qd, const float* goal, int32_t goal_stride,
                 const rmp2_obstacles* obs, const rmp2_rollout_cfg* cfg, const rmp2_outputs* out, int32_t R,
                 void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (int rc = refuse_staged(h, "rmp2_rollout", "the stage runs once per control step, outside the launch")) return rc;
  if (!cfg || cfg->n_control_steps < 1 || cfg->substeps < 0 || !(cfg->dt >= 0.f))
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "rollout: need n_control_steps >= 1, substeps >= 0, dt >= 0");
  if (obs && obs->mode == RMP2_OBS_EXPLICIT_PAIRS)
    return fail(h, RMP2_ERR_UNSUPPORTED, "rollout: explicit closest-point pairs go stale as the robots move; use a sphere mode");
  RolloutArgs ro{cfg->n_control_steps, cfg->substeps, cfg->dt, q, qd, 0};
  if (cfg->table_steps > 1) {
    if (cfg->table_steps != cfg->n_control_steps)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, "rollout: table_steps must be 0, 1 or n_control_steps");
    if (!obs || (obs->mode != RMP2_OBS_SHARED_SPHERES && obs->mode != RMP2_OBS_RAGGED_SPHERES))
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, "rollout: per-step obstacle tables need a sphere / capsule table mode");
    ro.table_stride = obs->n_spheres * (obs->primitive != RMP2_PRIM_SPHERE ? 8 : 4);
  }
  return step_impl(h, q, qd, goal, goal_stride, obs, out, ro, R, stream);
}

int rmp2_forward_kinematics(rmp2_handle* h, const float* q, float* T, int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (!q || !T || R < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "bad argument");
  if (R == 0 || h->n_frames == 0) return RMP2_OK;
  if (int rc = use_device(h)) return rc;
  const int blocks = (R + kWave - 1) / kWave;
  hipStream_t s = (hipStream_t)stream;
  with_slots(h->n_slots_full,
             [&](auto S) { hipLaunchKernelGGL((rmp2_fk_kernel<S>), dim3(blocks), dim3(kWave), 0, s, h->d_prog_full, q, T, R); });
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

int rmp2_closest_points(rmp2_handle* h, const float* q, const rmp2_obstacles* table, float* p_link, float* p_obs,
                        int32_t R, void* stream) {
  return rmp2_closest_points_links(h, q, table, nullptr, p_link, p_obs, R, stream);
}

int rmp2_closest_points_links(rmp2_handle* h, const float* q, const rmp2_obstacles* table, const float* link_capsules,
                              float* p_link, float* p_obs, int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (!q || !table || !p_link || !p_obs || R < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "bad argument");
  if (table->mode != RMP2_OBS_SHARED_SPHERES || table->n_spheres < 0 || (table->n_spheres > 0 && !table->spheres))
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "closest_points needs a SHARED_SPHERES primitive table");
  if (table->primitive != RMP2_PRIM_SPHERE && table->primitive != RMP2_PRIM_CAPSULE && table->primitive != RMP2_PRIM_CYLINDER)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "unknown obstacle primitive");
  if (R == 0 || !h->has_distance || table->n_spheres == 0) return RMP2_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = use_device(h)) return rc;
  // pair layout of the arrays written here: the i-th distance leaf owns pairs [i*K, (i+1)*K)
  rmp2_obstacles lay;
  explicit_pairs(h->distance_leaves, [table](int) { return table->n_spheres; }, p_link, p_obs, nullptr, lay);
  if (!h->pair_begin_valid || std::memcmp(h->h_pair_begin, lay.pair_begin, sizeof(h->h_pair_begin)) != 0) {
    std::memcpy(h->h_pair_begin, lay.pair_begin, sizeof(h->h_pair_begin));
    HIP_TRY(h, hipMemcpyAsync(h->d_pair_begin, h->h_pair_begin, sizeof(h->h_pair_begin), hipMemcpyHostToDevice, s));
    h->pair_begin_valid = true;
  }
  ObsArgs o = shared_table_args(table);
  o.n_pairs = lay.n_pairs;
  o.pair_begin = h->d_pair_begin;
  const int n_dist = (int)h->distance_leaves.size();
  const size_t seg_bytes = sizeof(float4) * 2 * kClosestRobots * n_dist;
  if (seg_bytes <= 64 * 1024 && h->kernel_choice != 1) {  // (more distance leaves than that, or RMP2_KERNEL=lane: a lane per robot)
    const int wblocks = (R + kClosestRobots - 1) / kClosestRobots;
#define RMP2_CLOSEST_WAVE_(LINK_, CAPS_)                                                                                \
    hipLaunchKernelGGL((rmp2_closest_wave_kernel<S, LINK_, CAPS_>), dim3(wblocks), dim3(kWave), seg_bytes, s, h->d_prog, q, o,   \
                       link_capsules, n_dist, p_link, p_obs, R)
    with_slots(h->n_slots, [&](auto S) {
      if (link_capsules && o.capsule) RMP2_CLOSEST_WAVE_(true, true);
      else if (link_capsules) RMP2_CLOSEST_WAVE_(true, false);
      else if (o.capsule) RMP2_CLOSEST_WAVE_(false, true);
      else RMP2_CLOSEST_WAVE_(false, false);
    });
#undef RMP2_CLOSEST_WAVE_
    HIP_TRY(h, hipGetLastError());
    return RMP2_OK;
  }
  const int blocks = (R + kWave - 1) / kWave;
  with_slots(h->n_slots, [&](auto S) {
    hipLaunchKernelGGL((rmp2_closest_kernel<S>), dim3(blocks), dim3(kWave), 0, s, h->d_prog, q, o, link_capsules, p_link, p_obs, R);
  });
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

int rmp2_set_self_collision(rmp2_handle* h, int32_t n_pairs, const int32_t* pairs, const float* capsules) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (n_pairs < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "n_pairs < 0");
  if (n_pairs == 0 || !pairs) {   // off (either geometry): the handle steps as one on which this was never called
    h->self_n_pairs = 0;
    h->self_counts.clear();
    h->self_hulls = false;
    return RMP2_OK;
  }
  if (h->hull_n > 0)
    return fail(h, RMP2_ERR_UNSUPPORTED, "self collision together with link hulls: not supported (turn the hulls off first)");
  if (n_pairs > RMP2_MAX_SELF_PAIRS)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "self collision: at most " + std::to_string(RMP2_MAX_SELF_PAIRS) + " pairs, got " +
                                                  std::to_string(n_pairs));
  if (!capsules) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "self collision: capsules [n_frames + 1][8] are required");
  const int F = h->n_frames, L = (int)h->pair_leaves.size();
  SelfProg sp;
  std::memset(&sp, 0, sizeof(sp));
  for (int l = 0; l < RMP2_MAX_LEAVES; ++l) sp.ord_of_leaf[l] = sp.dord[l] = -1;
  for (int f = 0; f < RMP2_MAX_FRAMES; ++f) sp.b_slot_of_frame[f] = -1;
  sp.base_slot = -1;
  sp.n_leaves = L;
  sp.n_dist = (int)h->distance_leaves.size();
  for (int o = 0, nd = 0; o < L; ++o) {
    sp.ord_of_leaf[h->pair_leaves[o]] = o;
    sp.dord[o] = h->pair_leaf_point[o] ? -1 : nd++;
  }
  std::vector<std::vector<int>> by_leaf;
  if (int rc = group_self_pairs(h, n_pairs, pairs, by_leaf, [](int, int, int) { return RMP2_OK; })) return rc;
  for (int f = 0; f <= F; ++f)
    for (int c = 0; c < 8; ++c)
      if (!std::isfinite(capsules[8 * f + c]) || (c == 3 && capsules[8 * f + c] < 0.f))
        return fail(h, RMP2_ERR_INVALID_ARGUMENT, "self collision: capsule " + std::to_string(f) + " is not finite or has a negative radius");
  std::vector<int> counts(L);
  int j = 0;
  for (int o = 0; o < L; ++o) {
    sp.self_begin[o] = j;
    counts[o] = (int)by_leaf[o].size();
    const float* lc = capsules + 8 * h->pair_leaf_frame[o];
    for (int c = 0; c < 8; ++c) sp.leaf_cap[o][c] = lc[c];
    for (int b : by_leaf[o]) {
      int& slot = b < 0 ? sp.base_slot : sp.b_slot_of_frame[b];
      if (slot < 0) {
        slot = sp.n_b++;
        const float* bc = capsules + 8 * (b < 0 ? F : b);
        for (int c = 0; c < 8; ++c) sp.b_cap[slot][c] = bc[c];
      }
      sp.pair_b[j++] = slot;
    }
  }
  sp.self_begin[L] = j;
  sp.n_pairs = j;
  // the stage's LDS: kClosestRobots robots' records, obstacle segments included
  const size_t lds = sizeof(float4) * kClosestRobots * (size_t)self_lds_records(sp.n_dist, L, sp.n_b);
  if (lds > 64 * 1024)
    return fail(h, RMP2_ERR_UNSUPPORTED, "self collision: the stage's records need " + std::to_string(lds) + " bytes of LDS (> 64 KiB)");
  if (int rc = use_device(h)) return rc;
  if (!h->d_self) HIP_TRY(h, hipMalloc(&h->d_self, sizeof(SelfProg)));
  HIP_TRY(h, hipMemcpy(h->d_self, &sp, sizeof(SelfProg), hipMemcpyHostToDevice));   // (synchronous: no launch still reads the old list)
  h->self_n_b = sp.n_b;
  h->self_counts = counts;
  h->self_n_pairs = n_pairs;
  h->self_hulls = false;   // (capsules replace hull self pairs)
  return RMP2_OK;
}

int rmp2_self_pairs(rmp2_handle* h, const float* q, float* p_link, float* p_obs, float* dist, int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (h->self_n_pairs == 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "self collision is off: rmp2_set_self_collision first");
  if (!q || !p_link || !p_obs || R < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "bad argument");
  bool point_pairs = false;
  for (size_t o = 0; o < h->pair_leaves.size(); ++o) point_pairs = point_pairs || (h->pair_leaf_point[o] && h->self_counts[o] > 0);
  if (point_pairs && !dist) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "attached-point leaves have self pairs: dist is required");
  if (R == 0) return RMP2_OK;
  if (int rc = use_device(h)) return rc;
  if (h->self_hulls) return launch_self_hull_stage(h, q, nullptr, p_link, p_obs, dist, h->self_n_pairs, R, (hipStream_t)stream);
  return launch_self_stage(h, q, nullptr, p_link, p_obs, dist, h->self_n_pairs, R, (hipStream_t)stream);
}

// The hull arrays of both hull setters (include/rmp2.h rmp2_set_link_hulls): n entries back to back, each with at most
// RMP2_MAX_HULL_VERTICES vertices and RMP2_MAX_HULL_FACES face planes -- at least one of each, or (empty_ok) neither --, finite vertices,
// unit normals and finite offsets.  `what` names the feature in the messages ("link hulls"), `entry` one entry ("link hull").
static int check_hulls(rmp2_handle* h, const char* what, const char* entry, bool empty_ok, int n, const int32_t* vert_offset,
                       const float* verts, const int32_t* face_offset, const float* planes) {
  const std::string w = what;
  if (!vert_offset || !verts || !face_offset || !planes) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": null array");
  if (vert_offset[0] != 0 || face_offset[0] != 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": offsets must start at 0");
  for (int e = 0; e < n; ++e) {
    const int nv = vert_offset[e + 1] - vert_offset[e], nf = face_offset[e + 1] - face_offset[e];
    if (empty_ok ? (nv < 0 || nf < 0 || (nv == 0) != (nf == 0)) : (nv < 1 || nf < 1))
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, std::string(entry) + " " + std::to_string(e) +
                                                    (empty_ok ? ": needs vertices and face planes, or neither"
                                                              : ": needs at least one vertex and one face plane"));
    if (nv > RMP2_MAX_HULL_VERTICES || nf > RMP2_MAX_HULL_FACES)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, std::string(entry) + " " + std::to_string(e) + ": " + std::to_string(nv) + " vertices / " +
                                                    std::to_string(nf) + " faces, at most RMP2_MAX_HULL_VERTICES = " +
                                                    std::to_string(RMP2_MAX_HULL_VERTICES) + " / RMP2_MAX_HULL_FACES = " +
                                                    std::to_string(RMP2_MAX_HULL_FACES));
  }
  for (size_t i = 0; i < (size_t)vert_offset[n]; ++i)
    if (!std::isfinite(verts[3 * i]) || !std::isfinite(verts[3 * i + 1]) || !std::isfinite(verts[3 * i + 2]))
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": vertex " + std::to_string(i) + " is not finite");
  for (size_t i = 0; i < (size_t)face_offset[n]; ++i) {
    const float* pl = planes + 4 * i;
    const double n2 = (double)pl[0] * pl[0] + (double)pl[1] * pl[1] + (double)pl[2] * pl[2];
    if (!std::isfinite(pl[3]) || !(std::fabs(n2 - 1.0) <= 1e-4))
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, w + ": plane " + std::to_string(i) + " needs a unit normal and a finite offset");
  }
  return RMP2_OK;
}

// Uploads the handle's hull arrays (rmp2_host.h: one set, for whichever hull geometry is on) and its HullProg.  Synchronous copies:
// no launch still reads the old hulls.
static int upload_hulls(rmp2_handle* h, const std::vector<float4>& hv, const std::vector<float4>& hpl, const HullProg& hp) {
  if (int rc = use_device(h)) return rc;
  const size_t nv = std::max<size_t>(hv.size(), 1), nf = std::max<size_t>(hpl.size(), 1);
  if (nv > h->hull_verts_cap) {
    h->hull_verts_cap = 0;
    if (int rc = realloc_device(h, &h->d_hull_verts, sizeof(float4) * nv)) return rc;
    h->hull_verts_cap = nv;
  }
  if (nf > h->hull_planes_cap) {
    h->hull_planes_cap = 0;
    if (int rc = realloc_device(h, &h->d_hull_planes, sizeof(float4) * nf)) return rc;
    h->hull_planes_cap = nf;
  }
  if (!h->d_hull) HIP_TRY(h, hipMalloc(&h->d_hull, sizeof(HullProg)));
  if (!hv.empty()) HIP_TRY(h, hipMemcpy(h->d_hull_verts, hv.data(), sizeof(float4) * hv.size(), hipMemcpyHostToDevice));
  if (!hpl.empty()) HIP_TRY(h, hipMemcpy(h->d_hull_planes, hpl.data(), sizeof(float4) * hpl.size(), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(h->d_hull, &hp, sizeof(HullProg), hipMemcpyHostToDevice));
  return RMP2_OK;
}

int rmp2_set_link_hulls(rmp2_handle* h, int32_t n_hulls, const int32_t* vert_offset, const float* verts, const int32_t* face_offset,
                        const float* planes) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (n_hulls < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "n_hulls < 0");
  if (n_hulls == 0) {   // off: the handle steps as one on which this was never called
    h->hull_n = 0;
    return RMP2_OK;
  }
  if (h->self_n_pairs > 0)
    return fail(h, RMP2_ERR_UNSUPPORTED, "link hulls together with self collision: not supported (turn self collision off first)");
  const int L = (int)h->pair_leaves.size();
  if (n_hulls != L)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "link hulls: one hull per distance / attached-point leaf (" + std::to_string(L) + "), got " +
                                                  std::to_string(n_hulls));
  if (int rc = check_hulls(h, "link hulls", "link hull", false, L, vert_offset, verts, face_offset, planes)) return rc;
  HullProg hp;
  std::memset(&hp, 0, sizeof(hp));
  hp.n_leaves = L;
  for (int l = 0; l < RMP2_MAX_LEAVES; ++l) hp.ord_of_leaf[l] = -1;
  for (int o = 0; o <= L; ++o) {
    if (o < L) hp.ord_of_leaf[h->pair_leaves[o]] = o, hp.is_point[o] = h->pair_leaf_point[o];
    hp.vert_off[o] = vert_offset[o], hp.face_off[o] = face_offset[o];
  }
  std::vector<float4> hv(vert_offset[L]), hpl(face_offset[L]);
  for (size_t i = 0; i < hv.size(); ++i) hv[i] = make_float4(verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], 0.f);
  for (size_t i = 0; i < hpl.size(); ++i) hpl[i] = make_float4(planes[4 * i], planes[4 * i + 1], planes[4 * i + 2], planes[4 * i + 3]);
  if (int rc = upload_hulls(h, hv, hpl, hp)) return rc;
  h->hull_n = L;
  return RMP2_OK;
}

int rmp2_set_self_collision_hulls(rmp2_handle* h, int32_t n_pairs, const int32_t* pairs, int32_t n_hulls, const int32_t* vert_offset,
                                  const float* verts, const int32_t* face_offset, const float* planes) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (n_pairs < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "n_pairs < 0");
  if (n_pairs == 0 || !pairs) return rmp2_set_self_collision(h, 0, nullptr, nullptr);   // off (either geometry)
  if (h->hull_n > 0)
    return fail(h, RMP2_ERR_UNSUPPORTED, "hull self pairs together with link hulls: not supported (turn the link hulls off first; the "
                                         "hull self pairs form the obstacle pairs on the same hulls)");
  if (n_pairs > RMP2_MAX_SELF_PAIRS)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "self collision: at most " + std::to_string(RMP2_MAX_SELF_PAIRS) + " pairs, got " +
                                                  std::to_string(n_pairs));
  const int F = h->n_frames, L = (int)h->pair_leaves.size();
  if (n_hulls != F + 1)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "hull self pairs: one hull entry per frame and the base (" + std::to_string(F + 1) +
                                                  "), got " + std::to_string(n_hulls));
  if (int rc = check_hulls(h, "hull self pairs", "hull entry", true, F + 1, vert_offset, verts, face_offset, planes)) return rc;
  // the pairs (rmp2_set_self_collision's rule, and no pair on an empty entry), grouped by ordinal
  auto entry_empty = [&](int e) { return vert_offset[e + 1] == vert_offset[e]; };
  std::vector<std::vector<int>> by_leaf;
  int rc = group_self_pairs(h, n_pairs, pairs, by_leaf, [&](int k, int o, int b) {
    const int ea = h->pair_leaf_frame[o], eb = b < 0 ? F : b;
    if (!entry_empty(ea) && !entry_empty(eb)) return RMP2_OK;
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "self pair " + std::to_string(k) + ": its hull entry " +
                                                  std::to_string(entry_empty(ea) ? ea : eb) + " is empty");
  });
  if (rc) return rc;
  // device arrays: the pair leaves' hulls first, in ordinal order (the obstacle half's HullProg), then every other non-empty entry
  HullProg hp;
  std::memset(&hp, 0, sizeof(hp));
  hp.n_leaves = L;
  for (int l = 0; l < RMP2_MAX_LEAVES; ++l) hp.ord_of_leaf[l] = -1;
  SelfHullProg sp;
  std::memset(&sp, 0, sizeof(sp));
  for (int f = 0; f < RMP2_MAX_FRAMES; ++f) sp.slot_of_frame[f] = -1;
  std::vector<float4> hv, hpl;
  std::vector<int> placed(F + 1, -1);
  auto append = [&](int e) {
    for (int i = vert_offset[e]; i < vert_offset[e + 1]; ++i) hv.push_back(make_float4(verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], 0.f));
    for (int i = face_offset[e]; i < face_offset[e + 1]; ++i)
      hpl.push_back(make_float4(planes[4 * i], planes[4 * i + 1], planes[4 * i + 2], planes[4 * i + 3]));
  };
  auto place = [&](int e) {   // the copy the self stage reads entry e from
    placed[e] = 1;
    sp.hv0[e] = (int)hv.size(), sp.hf0[e] = (int)hpl.size();
    sp.hnv[e] = vert_offset[e + 1] - vert_offset[e], sp.hnf[e] = face_offset[e + 1] - face_offset[e];
    append(e);
  };
  bool leaf_empty = false;
  for (int o = 0; o < L; ++o) {   // (two leaves on one frame share nothing here: each gets its own copy, as rmp2_set_link_hulls)
    const int e = h->pair_leaf_frame[o];
    hp.ord_of_leaf[h->pair_leaves[o]] = o;
    hp.is_point[o] = h->pair_leaf_point[o];
    hp.vert_off[o] = (int)hv.size(), hp.face_off[o] = (int)hpl.size();
    leaf_empty = leaf_empty || entry_empty(e);
    if (placed[e] < 0) place(e);
    else append(e);
  }
  hp.vert_off[L] = (int)hv.size(), hp.face_off[L] = (int)hpl.size();
  for (int e = 0; e <= F; ++e)
    if (placed[e] < 0 && !entry_empty(e)) place(e);
  std::vector<int> counts(L);
  int j = 0;
  auto slot_of = [&](int f) {
    if (sp.slot_of_frame[f] < 0) sp.slot_of_frame[f] = sp.n_slots++;
    return sp.slot_of_frame[f];
  };
  for (int o = 0; o < L; ++o) {
    hp.extra_before[o] = j;
    counts[o] = (int)by_leaf[o].size();
    sp.is_point[o] = h->pair_leaf_point[o];
    for (int b : by_leaf[o]) {
      const int fa = h->pair_leaf_frame[o];
      sp.pair_leaf[j] = o;
      sp.pair_sa[j] = slot_of(fa);
      sp.pair_sb[j] = b < 0 ? -1 : slot_of(b);
      sp.pair_ea[j] = fa;
      sp.pair_eb[j] = b < 0 ? F : b;
      ++j;
    }
  }
  sp.n_pairs = j;
  hp.n_extra = j;
  if ((rc = upload_hulls(h, hv, hpl, hp))) return rc;
  if (!h->d_shull) HIP_TRY(h, hipMalloc(&h->d_shull, sizeof(SelfHullProg)));
  HIP_TRY(h, hipMemcpy(h->d_shull, &sp, sizeof(SelfHullProg), hipMemcpyHostToDevice));   // (synchronous: no launch still reads it)
  h->shull_slots = sp.n_slots;
  h->shull_leaf_empty = leaf_empty;
  h->self_counts = counts;
  h->self_n_pairs = n_pairs;
  h->self_hulls = true;
  return RMP2_OK;
}

int rmp2_closest_points_hulls(rmp2_handle* h, const float* q, const rmp2_obstacles* table, float* p_link, float* p_obs, float* dist,
                              int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (h->hull_n == 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "link hulls are off: rmp2_set_link_hulls first");
  if (!q || !table || !p_link || !p_obs || R < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "bad argument");
  if (int rc = check_hull_table(h, table)) return rc;
  if (h->has_point && !dist) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "the set has attached-point leaves: dist is required");
  if (R == 0 || table->n_spheres == 0) return RMP2_OK;
  if (int rc = use_device(h)) return rc;
  return launch_hull_stage(h, q, table, p_link, p_obs, dist, R, (hipStream_t)stream);
}

static int differentiate_impl(rmp2_handle* h, const float* q, const float* qd, int32_t frame, float* x, float* xd, float* J,
                              float* c, int32_t R, void* stream, int euler) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (!q || !qd || !x || !xd || !J || !c || R < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "bad argument");
  if (frame < 0 || frame >= h->n_frames) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "frame out of range");
  if (R == 0) return RMP2_OK;
  if (int rc = use_device(h)) return rc;
  hipStream_t s = (hipStream_t)stream;
  // The per-robot scratch belongs to the handle: the differentiate entry points are single-stream per handle
  // (include/rmp2.h).  It grows monotonically; hipFree synchronises the device, so no launch still reads the old one.
  if ((size_t)R > h->scratch_robots) {
    h->scratch_robots = 0;
    if (int rc = realloc_device(h, &h->d_scratch, sizeof(float) * 6 * RMP2_MAX_DOF * (size_t)R)) return rc;
    h->scratch_robots = (size_t)R;
  }
  const int blocks = (R + kWave - 1) / kWave;
  with_slots(h->n_slots_full, [&](auto S) {
    hipLaunchKernelGGL((rmp2_diff_kernel<S>), dim3(blocks), dim3(kWave), 0, s, h->d_prog_full, q, qd, frame, x, xd, J, c,
                       h->d_scratch, R, euler);
  });
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

int rmp2_differentiate(rmp2_handle* h, const float* q, const float* qd, int32_t frame, float* x, float* xd, float* J,
                       float* c, int32_t R, void* stream) {
  return differentiate_impl(h, q, qd, frame, x, xd, J, c, R, stream, 0);
}

int rmp2_differentiate_euler(rmp2_handle* h, const float* q, const float* qd, int32_t frame, float* x, float* xd,
                             float* J, float* c, int32_t R, void* stream) {
  return differentiate_impl(h, q, qd, frame, x, xd, J, c, R, stream, 1);
}

int rmp2_set_inertials(rmp2_handle* h, int32_t n_frames, const float* inertials, const float* gravity) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (n_frames < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inertials: n_frames < 0");
  if (n_frames == 0) {   // off: rmp2_inverse_dynamics is refused again
    h->inert_n = 0;
    return RMP2_OK;
  }
  if (n_frames != h->n_frames)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inertials: one record per frame (" + std::to_string(h->n_frames) + "), got " +
                                                  std::to_string(n_frames));
  if (!inertials) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inertials: null array");
  float acc[3] = {0.f, 0.f, 9.81f};
  if (gravity) {
    for (int k = 0; k < 3; ++k) {
      if (!std::isfinite(gravity[k])) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inertials: gravity is not finite");
      acc[k] = -gravity[k];
    }
  }
  static const char* const kField[kInertialFloats] = {"m", "cx", "cy", "cz", "Ixx", "Iyy", "Izz", "Ixy", "Ixz", "Iyz"};
  for (int f = 0; f < n_frames; ++f) {
    const float* r = inertials + (size_t)f * kInertialFloats;
    for (int k = 0; k < kInertialFloats; ++k)
      if (!std::isfinite(r[k]))
        return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inertials: frame " + std::to_string(f) + ": " + kField[k] + " is not finite");
    if (r[0] < 0.f) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inertials: frame " + std::to_string(f) + ": mass < 0");
    for (int k = 4; k < 7; ++k)
      if (r[k] < 0.f)
        return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inertials: frame " + std::to_string(f) + ": " + kField[k] + " < 0");
  }
  if (int rc = use_device(h)) return rc;
  if (!h->d_inert) HIP_TRY(h, hipMalloc(&h->d_inert, sizeof(float) * kInertialFloats * RMP2_MAX_FRAMES));
  // (a synchronous copy: no launch still reads the old table)
  HIP_TRY(h, hipMemcpy(h->d_inert, inertials, sizeof(float) * kInertialFloats * n_frames, hipMemcpyHostToDevice));
  for (int k = 0; k < 3; ++k) h->base_acc[k] = acc[k];
  h->inert_n = n_frames;
  return RMP2_OK;
}

int rmp2_inverse_dynamics(rmp2_handle* h, const float* q, const float* qd, const float* qdd, float* tau, int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (R < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inverse dynamics: R < 0");
  if (h->inert_n == 0)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inverse dynamics: no inertial table on this handle (call rmp2_set_inertials first)");
  if (R == 0) return RMP2_OK;
  if (!q || !qd || !qdd || !tau) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "inverse dynamics: null array");
  if (int rc = use_device(h)) return rc;
  hipStream_t s = (hipStream_t)stream;
  switch (h->n_template) {
    case 2: launch_inverse_dynamics<2>(h, q, qd, qdd, tau, R, s); break;
    case 9: launch_inverse_dynamics<9>(h, q, qd, qdd, tau, R, s); break;
    default: launch_inverse_dynamics<16>(h, q, qd, qdd, tau, R, s); break;
  }
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

int rmp2_mass_matrix(rmp2_handle* h, const float* q, float* M, int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (R < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "mass matrix: R < 0");
  if (h->inert_n == 0)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "mass matrix: no inertial table on this handle (call rmp2_set_inertials first)");
  if (R == 0) return RMP2_OK;
  if (!q || !M) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "mass matrix: null array");
  if (int rc = use_device(h)) return rc;
  hipStream_t s = (hipStream_t)stream;
  switch (h->n_template) {
    case 2: launch_mass_matrix<2>(h, q, M, R, s); break;
    case 9: launch_mass_matrix<9>(h, q, M, R, s); break;
    default: launch_mass_matrix<16>(h, q, M, R, s); break;
  }
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

int rmp2_forward_dynamics(rmp2_handle* h, const float* q, const float* qd, const float* tau, float* qdd, int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  // (one evaluation of the step's kernel in the torque drive; q and qd are only read)
  return dynamics_step_impl(h, "forward dynamics", const_cast<float*>(q), const_cast<float*>(qd), tau, 0, nullptr, 0.f, 1, 0, qdd,
                            nullptr, R, stream);
}

int rmp2_dynamics_step(rmp2_handle* h, float* q, float* qd, const float* u, int32_t drive, const float* tau_limit, float dt,
                       int32_t substeps, float* qdd_out, float* tau_out, int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (int rc = step_args_check(h, "dynamics step", drive, substeps, dt)) return rc;
  return dynamics_step_impl(h, "dynamics step", q, qd, u, drive == RMP2_DRIVE_ACCEL, tau_limit, dt, substeps, 1, qdd_out, tau_out, R,
                            stream);
}

int rmp2_dynamics_step_stops(rmp2_handle* h, float* q, float* qd, const float* u, int32_t drive, const float* tau_limit,
                             const float* q_lower, const float* q_upper, float dt, int32_t substeps, float* qdd_out, float* tau_out,
                             float* stop_out, uint32_t* status_out, int32_t R, void* stream) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  const char* what = "dynamics step with stops";
  if (int rc = step_args_check(h, what, drive, substeps, dt)) return rc;
  bool launch;
  if (int rc = step_rows_check(h, what, q, qd, u, q_lower && q_upper, R, launch)) return rc;
  if (!launch) return RMP2_OK;
  hipStream_t s = (hipStream_t)stream;
  const int accel = drive == RMP2_DRIVE_ACCEL;
  switch (h->n_template) {
    case 2: launch_dynamics_step_stops<2>(h, q, qd, u, accel, tau_limit, q_lower, q_upper, dt, substeps, qdd_out, tau_out, stop_out, status_out, R, s); break;
    case 9: launch_dynamics_step_stops<9>(h, q, qd, u, accel, tau_limit, q_lower, q_upper, dt, substeps, qdd_out, tau_out, stop_out, status_out, R, s); break;
    default: launch_dynamics_step_stops<16>(h, q, qd, u, accel, tau_limit, q_lower, q_upper, dt, substeps, qdd_out, tau_out, stop_out, status_out, R, s); break;
  }
  HIP_TRY(h, hipGetLastError());
  return RMP2_OK;
}

int rmp2_set_contact_capsules(rmp2_handle* h, int32_t n_frames, const float* capsules) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (n_frames < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "contact capsules: n_frames < 0");
  if (n_frames == 0 || !capsules) {   // off: rmp2_dynamics_step_contacts is refused again
    h->contact_n = 0;
    return RMP2_OK;
  }
  if (n_frames != h->n_frames)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "contact capsules: one record per frame (" + std::to_string(h->n_frames) + "), got " +
                                                  std::to_string(n_frames));
  for (int f = 0; f < n_frames; ++f) {
    const float* r = capsules + (size_t)f * 8;
    for (int k = 0; k < 8; ++k)
      if (!std::isfinite(r[k]))
        return fail(h, RMP2_ERR_INVALID_ARGUMENT, "contact capsules: frame " + std::to_string(f) + ": a value is not finite");
    if (r[3] < 0.f) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "contact capsules: frame " + std::to_string(f) + ": radius < 0");
  }
  if (int rc = use_device(h)) return rc;
  if (!h->d_contact_caps) HIP_TRY(h, hipMalloc(&h->d_contact_caps, sizeof(float) * 8 * RMP2_MAX_FRAMES));
  // (a synchronous copy: no launch still reads the old table)
  HIP_TRY(h, hipMemcpy(h->d_contact_caps, capsules, sizeof(float) * 8 * n_frames, hipMemcpyHostToDevice));
  h->contact_n = n_frames;
  return RMP2_OK;
}

int rmp2_set_contact_self_pairs(rmp2_handle* h, int32_t n_pairs, const int32_t* pairs) {
  if (!h) return RMP2_ERR_INVALID_ARGUMENT;
  if (n_pairs < 0) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "contact self pairs: n_pairs < 0");
  if (n_pairs == 0) {   // off: rmp2_dynamics_step_contacts_self is the capsules call again
    h->contact_self_n = 0;
    return RMP2_OK;
  }
  if (!pairs) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "contact self pairs: null pair list with n_pairs > 0");
  const int n_ops = (int)h->full_op_frame.size();
  std::vector<int> op_of(h->n_frames, -1);   // the op that visits each frame
  for (int k = 0; k < n_ops; ++k)
    if (h->full_op_frame[k] >= 0 && h->full_op_frame[k] < h->n_frames) op_of[h->full_op_frame[k]] = k;
  const int max_pairs = RMP2_MAX_FRAMES * (RMP2_MAX_FRAMES - 1) / 2;
  if (n_pairs > max_pairs) return fail(h, RMP2_ERR_INVALID_ARGUMENT, "contact self pairs: more pairs than there are frame pairs");
  std::vector<std::vector<int>> partners(n_ops);   // per link op: its partners' ops, in the caller's order
  std::vector<int32_t> slot(n_ops, -1);
  std::vector<char> seen((size_t)h->n_frames * h->n_frames, 0);
  int n_slots = 0;
  for (int p = 0; p < n_pairs; ++p) {
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    const std::string at = "contact self pairs: pair " + std::to_string(p);
    if (i < 0 || i >= h->n_frames || j < 0 || j >= h->n_frames || op_of[i] < 0 || op_of[j] < 0)
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, at + ": a frame is out of range");
    if (i == j) return fail(h, RMP2_ERR_INVALID_ARGUMENT, at + ": a frame against itself");
    if (seen[(size_t)i * h->n_frames + j]) return fail(h, RMP2_ERR_INVALID_ARGUMENT, at + ": given twice");
    seen[(size_t)i * h->n_frames + j] = seen[(size_t)j * h->n_frames + i] = 1;
    const int kf = std::max(op_of[i], op_of[j]), ke = std::min(op_of[i], op_of[j]);
    if (h->full_op_anc[kf] == h->full_op_anc[ke])
      return fail(h, RMP2_ERR_INVALID_ARGUMENT, at + ": the two frames are rigidly connected (the same dofs move both)");
    if (slot[ke] < 0) slot[ke] = n_slots++;
    partners[kf].push_back(ke);
  }
  if (n_slots > RMP2_MAX_CONTACT_SELF_FRAMES)
    return fail(h, RMP2_ERR_INVALID_ARGUMENT, "contact self pairs: " + std::to_string(n_slots) + " distinct partner frames, at most " +
                                                  std::to_string(RMP2_MAX_CONTACT_SELF_FRAMES));
  std::vector<int32_t> tab(slot);   // slot [n_ops] | begin [n_ops + 1] | rec [n_pairs][4]
  int at = 0;
  for (int k = 0; k < n_ops; ++k) {
    tab.push_back(at);
    at += (int)partners[k].size();
  }
  tab.push_back(at);
  for (int k = 0; k < n_ops; ++k)
    for (int ke : partners[k]) {
      const uint32_t af = h->full_op_anc[k], ae = h->full_op_anc[ke];
      tab.insert(tab.end(), {slot[ke], h->full_op_frame[ke], (int32_t)(af & ~ae), (int32_t)(ae & ~af)});
    }
  if (int rc = use_device(h)) return rc;
  if (!h->d_contact_self)
    HIP_TRY(h, hipMalloc(&h->d_contact_self, sizeof(int32_t) * (2 * RMP2_MAX_FRAMES + 1 + 4 * max_pairs)));
  // (a synchronous copy: no launch still reads the old tables)
  HIP_TRY(h, hipMemcpy(h->d_contact_self, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice));
  h->contact_self_n = n_pairs;
  return RMP2_OK;
}

int rmp2_dynamics_step_contacts(rmp2_handle* h, float* q, float* qd, const float* u, int32_t drive, const float* tau_limit,
                                const float* q_lower, const float* q_upper, const float* spheres, int32_t K, float d_act, float dt,
                                int32_t substeps, float* qdd_out, float* tau_out, float* stop_out, float* contact_out,
                                float* contact_lambda, int32_t* contact_pair, uint32_t* status_out, int32_t R, void* stream) {
  ContactCall c = contact_call(q, qd, u, tau_limit, q_lower, q_upper, spheres, K, d_act, dt, substeps, qdd_out, tau_out, stop_out,
                               contact_out, contact_lambda, contact_pair, status_out, R);
  return contacts_step_impl(h, "dynamics step with contacts", kContactsTable, drive, c, stream);
}

int rmp2_dynamics_step_contacts_lists(rmp2_handle* h, float* q, float* qd, const float* u, int32_t drive, const float* tau_limit,
                                      const float* q_lower, const float* q_upper, const float* spheres, int32_t K,
                                      const int32_t* csr_offset, const int32_t* csr_index, float d_act, float dt, int32_t substeps,
                                      float* qdd_out, float* tau_out, float* stop_out, float* contact_out, float* contact_lambda,
                                      int32_t* contact_pair, uint32_t* status_out, int32_t R, void* stream) {
  ContactCall c = contact_call(q, qd, u, tau_limit, q_lower, q_upper, spheres, K, d_act, dt, substeps, qdd_out, tau_out, stop_out,
                               contact_out, contact_lambda, contact_pair, status_out, R);
  c.csr_offset = csr_offset, c.csr_index = csr_index;
  return contacts_step_impl(h, "dynamics step with contact lists", kContactsLists, drive, c, stream);
}

int rmp2_dynamics_step_contacts_planes(rmp2_handle* h, float* q, float* qd, const float* u, int32_t drive, const float* tau_limit,
                                       const float* q_lower, const float* q_upper, const float* spheres, int32_t K,
                                       const int32_t* csr_offset, const int32_t* csr_index, const float* planes, int32_t P,
                                       float d_act, float dt, int32_t substeps, float* qdd_out, float* tau_out, float* stop_out,
                                       float* contact_out, float* contact_lambda, int32_t* contact_pair, uint32_t* status_out,
                                       int32_t R, void* stream) {
  ContactCall c = contact_call(q, qd, u, tau_limit, q_lower, q_upper, spheres, K, d_act, dt, substeps, qdd_out, tau_out, stop_out,
                               contact_out, contact_lambda, contact_pair, status_out, R);
  c.csr_offset = csr_offset, c.csr_index = csr_index;
  c.planes = planes, c.P = P;
  return contacts_step_impl(h, "dynamics step with contact planes", kContactsPlanes, drive, c, stream);
}

int rmp2_dynamics_step_contacts_capsules(rmp2_handle* h, float* q, float* qd, const float* u, int32_t drive, const float* tau_limit,
                                         const float* q_lower, const float* q_upper, const float* spheres, int32_t K,
                                         const int32_t* csr_offset, const int32_t* csr_index, const float* planes, int32_t P,
                                         const float* obstacle_capsules, int32_t C, float d_act, float dt, int32_t substeps,
                                         float* qdd_out, float* tau_out, float* stop_out, float* contact_out, float* contact_lambda,
                                         int32_t* contact_pair, uint32_t* status_out, int32_t R, void* stream) {
  ContactCall c = contact_call(q, qd, u, tau_limit, q_lower, q_upper, spheres, K, d_act, dt, substeps, qdd_out, tau_out, stop_out,
                               contact_out, contact_lambda, contact_pair, status_out, R);
  c.csr_offset = csr_offset, c.csr_index = csr_index;
  c.planes = planes, c.P = P;
  c.capsules = obstacle_capsules, c.C = C;
  return contacts_step_impl(h, "dynamics step with contact capsules", kContactsCapsules, drive, c, stream);
}

int rmp2_dynamics_step_contacts_self(rmp2_handle* h, float* q, float* qd, const float* u, int32_t drive, const float* tau_limit,
                                     const float* q_lower, const float* q_upper, const float* spheres, int32_t K,
                                     const int32_t* csr_offset, const int32_t* csr_index, const float* planes, int32_t P,
                                     const float* obstacle_capsules, int32_t C, float d_act, float dt, int32_t substeps,
                                     float* qdd_out, float* tau_out, float* stop_out, float* contact_out, float* contact_lambda,
                                     int32_t* contact_pair, uint32_t* status_out, int32_t R, void* stream) {
  ContactCall c = contact_call(q, qd, u, tau_limit, q_lower, q_upper, spheres, K, d_act, dt, substeps, qdd_out, tau_out, stop_out,
                               contact_out, contact_lambda, contact_pair, status_out, R);
  c.csr_offset = csr_offset, c.csr_index = csr_index;
  c.planes = planes, c.P = P;
  c.capsules = obstacle_capsules, c.C = C;
  return contacts_step_impl(h, "dynamics step with self contacts", kContactsSelf, drive, c, stream);
}

int rmp2_dynamics_step_contacts_cylinders(rmp2_handle* h, float* q, float* qd, const float* u, int32_t drive, const float* tau_limit,
                                          const float* q_lower, const float* q_upper, const float* spheres, int32_t K,
                                          const int32_t* csr_offset, const int32_t* csr_index, const float* planes, int32_t P,
                                          const float* obstacle_capsules, int32_t C, const float* cylinders, int32_t Y,
                                          int32_t self_pairs, float d_act, float dt, int32_t substeps, float* qdd_out, float* tau_out,
                                          float* stop_out, float* contact_out, float* contact_lambda, int32_t* contact_pair,
                                          uint32_t* status_out, int32_t R, void* stream) {
  ContactCall c = contact_call(q, qd, u, tau_limit, q_lower, q_upper, spheres, K, d_act, dt, substeps, qdd_out, tau_out, stop_out,
                               contact_out, contact_lambda, contact_pair, status_out, R);
  c.csr_offset = csr_offset, c.csr_index = csr_index;
  c.planes = planes, c.P = P;
  c.capsules = obstacle_capsules, c.C = C;
  c.cylinders = cylinders, c.Y = Y, c.self_pairs = self_pairs;
  return contacts_step_impl(h, "dynamics step with contact cylinders", kContactsCylinders, drive, c, stream);
}

int rmp2_dynamics_step_contacts_cylinder_lists(rmp2_handle* h, float* q, float* qd, const float* u, int32_t drive,
                                               const float* tau_limit, const float* q_lower, const float* q_upper,
                                               const float* spheres, int32_t K, const int32_t* csr_offset, const int32_t* csr_index,
                                               const float* planes, int32_t P, const float* obstacle_capsules, int32_t C,
                                               const float* cylinders, int32_t Y, const int32_t* cyl_offset, const int32_t* cyl_index,
                                               int32_t self_pairs, float d_act, float dt, int32_t substeps, float* qdd_out,
                                               float* tau_out, float* stop_out, float* contact_out, float* contact_lambda,
                                               int32_t* contact_pair, uint32_t* status_out, int32_t R, void* stream) {
  ContactCall c = contact_call(q, qd, u, tau_limit, q_lower, q_upper, spheres, K, d_act, dt, substeps, qdd_out, tau_out, stop_out,
                               contact_out, contact_lambda, contact_pair, status_out, R);
  c.csr_offset = csr_offset, c.csr_index = csr_index;
  c.planes = planes, c.P = P;
  c.capsules = obstacle_capsules, c.C = C;
  c.cylinders = cylinders, c.Y = Y, c.self_pairs = self_pairs;
  c.cyl_offset = cyl_offset, c.cyl_index = cyl_index;
  return contacts_step_impl(h, "dynamics step with contact cylinder lists", kContactsCylinderLists, drive, c, stream);
}

}  // extern "C"

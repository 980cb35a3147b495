// rmp2_dynamics.h -- inverse dynamics of one fixed-base robot (include/rmp2.h rmp2_inverse_dynamics).
//
// The reference ends every control step with p.calculateInverseDynamics(q, qd, qdd) (simulation.py:369-386): the generalised
// forces tau = M(q) qdd + C(q, qd) qd + G(q) of the rigid-body tree described by the URDF's <inertial> data.  Here it is one
// forward walk over the unpruned program (the frames the FK entry points visit, rmp2_fk_kernel's save / restore slots):
//   - per frame, in world coordinates: the pose, the angular velocity w, the angular acceleration dw and the acceleration a of
//     the frame's origin, all with qdd included; the base accelerates by -g, which puts gravity into every body;
//   - the body wrench of the frame's link: F = m a_c (a_c the acceleration of its centre of mass c) and N = I_w dw + w x I_w w;
//   - its contribution to every dof j that moves the frame (DevOp::anc_mask), projected on joint j's screw:
//       tau_j += z_j . (c x F + N) + (o_j x z_j) . F   (revolute: the moment about the joint's axis through o_j)
//       tau_j += z_j . F                               (prismatic: the force along the axis)
//     the screws (z_j, o_j x z_j) -- (0, z_j) for a prismatic joint -- are stored when the walk passes joint j.
// No backward sweep and no per-frame storage beyond the save slots: 7 N floats per robot for the screws and the sums.
// Everything is fp32 (within the bound of include/rmp2.h; tests/test_inverse_dynamics_host.py measures it on the CPU).
//
// The inertial record of frame f (its child link, in the frame's coordinates): (m, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Ixz, Iyz),
// the tensor about the centre of mass.  Host-compilable (__host__ __device__) so that the same code runs on the CPU
// (tests/inverse_dynamics_driver.cpp).
#pragma once
#include <math.h>

#include "rmp2_device.h"

namespace rmp2 {

constexpr int kInertialFloats = 10;

__host__ __device__ inline void id_cross(const float a[3], const float b[3], float o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

__host__ __device__ inline float id_dot(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// running state of the walk (world coordinates)
struct IdState {
  float R[9];   // rotation, row-major
  float p[3];   // origin
  float w[3];   // angular velocity
  float dw[3];  // angular acceleration
  float a[3];   // linear acceleration of the origin (gravity included: the base accelerates by -g)
};

// One frame: s (the parent's state, ignored when from_base) -> this frame's state; z = the joint's world axis.
// The pose is visit_frame's (rmp2_device.h); the velocities carry qdd, which visit_frame's bias terms leave out.
__host__ __device__ inline void id_visit(IdState& s, const DevOp& op, float qv, float qdv, float qddv, bool from_base,
                                         const float base_acc[3], float z[3]) {
  const float ax[3] = {op.axis[0], op.axis[1], op.axis[2]};
  float Rl[9], tl[3];
  if (op.jtype == RMP2_JOINT_REVOLUTE) {
    // T_variable = [Rodrigues(axis, q) | 0]; Rodrigues = cos*I + sin*[u]x + (1-cos)*u u^T
    float sn, cs;
#if defined(__HIP_DEVICE_COMPILE__)
    sincosf(qv, &sn, &cs);
#else
    sn = sinf(qv);
    cs = cosf(qv);
#endif
    const float omc = 1.0f - cs;
    const float ut[9] = {0.f, -ax[2], ax[1], ax[2], 0.f, -ax[0], -ax[1], ax[0], 0.f};
    float Rv[9];
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) Rv[3 * r + k] = cs * (r == k ? 1.f : 0.f) + sn * ut[3 * r + k] + omc * (ax[r] * ax[k]);
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k)
        Rl[3 * r + k] = op.Tc[4 * r + 0] * Rv[k] + op.Tc[4 * r + 1] * Rv[3 + k] + op.Tc[4 * r + 2] * Rv[6 + k];
    for (int r = 0; r < 3; ++r) tl[r] = op.Tc[4 * r + 3];
  } else {
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) Rl[3 * r + k] = op.Tc[4 * r + k];
      tl[r] = op.Tc[4 * r + 3];
    }
    if (op.jtype == RMP2_JOINT_PRISMATIC) {
      const float tv[3] = {qv * ax[0], qv * ax[1], qv * ax[2]};
      for (int r = 0; r < 3; ++r)
        tl[r] = op.Tc[4 * r + 0] * tv[0] + op.Tc[4 * r + 1] * tv[1] + op.Tc[4 * r + 2] * tv[2] + op.Tc[4 * r + 3];
    }
  }
  float wp[3], dwp[3], ap[3], r[3];
  if (from_base) {
    for (int k = 0; k < 9; ++k) s.R[k] = Rl[k];
    for (int k = 0; k < 3; ++k) {
      s.p[k] = tl[k];
      r[k] = tl[k];
      wp[k] = dwp[k] = 0.f;
      ap[k] = base_acc[k];
    }
  } else {
    float Rn[9], pn[3];
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 3; ++k)
        Rn[3 * i + k] = s.R[3 * i + 0] * Rl[k] + s.R[3 * i + 1] * Rl[3 + k] + s.R[3 * i + 2] * Rl[6 + k];
      pn[i] = s.R[3 * i + 0] * tl[0] + s.R[3 * i + 1] * tl[1] + s.R[3 * i + 2] * tl[2] + s.p[i];
    }
    for (int k = 0; k < 3; ++k) {
      r[k] = pn[k] - s.p[k];
      s.p[k] = pn[k];
      wp[k] = s.w[k];
      dwp[k] = s.dw[k];
      ap[k] = s.a[k];
    }
    for (int k = 0; k < 9; ++k) s.R[k] = Rn[k];
  }
  for (int k = 0; k < 3; ++k) z[k] = s.R[3 * k + 0] * ax[0] + s.R[3 * k + 1] * ax[1] + s.R[3 * k + 2] * ax[2];
  // the origin is a point of the parent's link (plus the slide of a prismatic joint): a = a_p + dw_p x r + w_p x (w_p x r)
  float t1[3], t2[3], t3[3];
  id_cross(dwp, r, t1);
  id_cross(wp, r, t2);
  id_cross(wp, t2, t3);
  for (int k = 0; k < 3; ++k) {
    s.a[k] = ap[k] + t1[k] + t3[k];
    s.w[k] = wp[k];
    s.dw[k] = dwp[k];
  }
  if (op.jtype != RMP2_JOINT_FIXED) {
    const float u[3] = {qdv * z[0], qdv * z[1], qdv * z[2]};   // the joint's rate along its axis
    float wu[3];
    id_cross(wp, u, wu);
    if (op.jtype == RMP2_JOINT_REVOLUTE) {
      for (int k = 0; k < 3; ++k) {
        s.w[k] += u[k];
        s.dw[k] += qddv * z[k] + wu[k];
      }
    } else {
      for (int k = 0; k < 3; ++k) s.a[k] += qddv * z[k] + 2.f * wu[k];
    }
  }
}

// tau[0 .. n_dof) of one robot.  ops[0 .. n_ops): the unpruned program (every frame once, depth first); inert[F][10]: the frames'
// inertial records; base_acc = -g (world = base frame).  q / qd / qdd: the robot's rows.  A dof that no joint of the program owns
// gets 0; a non-finite input anywhere in the three rows makes every entry non-finite.
template <int N, int SLOTS>
__host__ __device__ inline void inverse_dynamics_robot(const DevOp* ops, int n_ops, int n_dof, const float* inert,
                                                       const float base_acc[3], const float* q, const float* qd, const float* qdd,
                                                       float* tau) {
  float sa[N][3], sl[N][3], acc[N];   // joint screws (angular, linear part) and the sums
#pragma unroll
  for (int j = 0; j < N; ++j) {
    acc[j] = 0.f;
    for (int k = 0; k < 3; ++k) sa[j][k] = sl[j][k] = 0.f;
  }
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
    float z[3];
    id_visit(cur, op, qi >= 0 ? q[qi] : 0.f, qi >= 0 ? qd[qi] : 0.f, qi >= 0 ? qdd[qi] : 0.f, op.restore == -2, base_acc, z);
    if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.save == s) slot[s] = cur;
    }
    if (qi >= 0) {   // this joint's screw, kept for the frames below it
      float oz[3];
      id_cross(cur.p, z, oz);
      const bool rev = op.jtype == RMP2_JOINT_REVOLUTE;
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (j == qi)
          for (int c = 0; c < 3; ++c) {
            sa[j][c] = rev ? z[c] : 0.f;
            sl[j][c] = rev ? oz[c] : z[c];
          }
    }
    // the link's wrench: F = m a_c, N = I_w dw + w x I_w w (formed in the frame's axes: I_w x = R (I (R^T x)))
    const float* in = inert + (size_t)op.frame * kInertialFloats;
    const float m = in[0];
    const float cl[3] = {in[1], in[2], in[3]};
    const float I[9] = {in[4], in[7], in[8], in[7], in[5], in[9], in[8], in[9], in[6]};
    float cw[3], wl[3], dwl[3];
    for (int i = 0; i < 3; ++i) {
      cw[i] = cur.R[3 * i + 0] * cl[0] + cur.R[3 * i + 1] * cl[1] + cur.R[3 * i + 2] * cl[2];
      wl[i] = cur.R[i] * cur.w[0] + cur.R[3 + i] * cur.w[1] + cur.R[6 + i] * cur.w[2];
      dwl[i] = cur.R[i] * cur.dw[0] + cur.R[3 + i] * cur.dw[1] + cur.R[6 + i] * cur.dw[2];
    }
    float t1[3], t2[3], t3[3], F[3], cb[3];
    id_cross(cur.dw, cw, t1);
    id_cross(cur.w, cw, t2);
    id_cross(cur.w, t2, t3);
    for (int i = 0; i < 3; ++i) {
      F[i] = m * (cur.a[i] + t1[i] + t3[i]);
      cb[i] = cur.p[i] + cw[i];
    }
    float Iw[3], Idw[3], gyr[3], Nl[3];
    for (int i = 0; i < 3; ++i) {
      Iw[i] = I[3 * i + 0] * wl[0] + I[3 * i + 1] * wl[1] + I[3 * i + 2] * wl[2];
      Idw[i] = I[3 * i + 0] * dwl[0] + I[3 * i + 1] * dwl[1] + I[3 * i + 2] * dwl[2];
    }
    id_cross(wl, Iw, gyr);
    for (int i = 0; i < 3; ++i) Nl[i] = Idw[i] + gyr[i];
    float M[3];   // moment about the world origin: c x F + R N_l
    id_cross(cb, F, M);
    for (int i = 0; i < 3; ++i) M[i] += cur.R[3 * i + 0] * Nl[0] + cur.R[3 * i + 1] * Nl[1] + cur.R[3 * i + 2] * Nl[2];
    const uint32_t mask = op.anc_mask;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if ((mask >> j) & 1u) acc[j] += id_dot(sa[j], M) + id_dot(sl[j], F);
  }
  // a non-finite input poisons the robot's whole row (x * 0 is NaN for NaN and Inf): also inputs the tree never reads
  float poison = 0.f;
  for (int j = 0; j < n_dof; ++j) poison += q[j] * 0.f + qd[j] * 0.f + qdd[j] * 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < n_dof) tau[j] = acc[j] + poison;
}

}  // namespace rmp2

// rmp2_contact_planes_tu.hip -- the kernels of rmp2_dynamics_step_contacts_planes (include/rmp2.h) and their launcher: the contact
// step of rmp2_contacts.h with half-space obstacles beside the spheres, the routines instantiated with PlaneTable.  Compiled twice,
// RMP2_TU_LIST = 0 (the shared sphere table) and 1 (per-robot lists over a pool), each a code object of its own: rmp2_hip.hip's and
// rmp2_contacts_lists_tu.hip's device code stays byte for byte what it is without this entry point.
#include <cfloat>
#include <cmath>

#include "rmp2_host.h"
#include "rmp2_contacts.h"

#ifndef RMP2_TU_LIST
#error "RMP2_TU_LIST must be 0 (table form) or 1 (list form)"
#endif

namespace rmp2 {

// One lane per robot, one wave per block; the per-lane storage in LDS as in rmp2_dynamics_step_contacts_kernel (no word added: the
// plane rows go into the same candidate slots).  planes [P][4] is read at uniform addresses.  LIST: csr_offset / csr_index as in
// rmp2_dynamics_step_contacts_lists_kernel; otherwise both are unused.
template <int N, int SLOTS, bool LIST>
__global__ void __launch_bounds__(kWave)
rmp2_dynamics_step_contacts_planes_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, float ax, float ay,
                                          float az, float* q, float* qd, const float* __restrict__ u, int accel,
                                          const float* __restrict__ lim, const float* __restrict__ qlo,
                                          const float* __restrict__ qhi, const float* __restrict__ caps,
                                          const float* __restrict__ spheres, int K, const int32_t* __restrict__ csr_offset,
                                          const int32_t* __restrict__ csr_index, const float* __restrict__ planes, int P, int F,
                                          float d_act, float dt, int substeps, float* __restrict__ qdd_out,
                                          float* __restrict__ tau_out, float* __restrict__ stop_out, float* __restrict__ contact_out,
                                          float* __restrict__ lambda_out, int32_t* __restrict__ pair_out,
                                          uint32_t* __restrict__ status_out, int R) {
  static_assert(contact_words(N) * kWave * sizeof(float) <= 65536, "the per-lane storage of one wave must fit 64 KiB of LDS");
  __shared__ float lds[contact_words(N) * kWave];
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  const int n_dof = prog->n_dof;
  const size_t row = (size_t)robot * n_dof;
  const size_t crow = (size_t)robot * kMaxContacts;
  const float base_acc[3] = {ax, ay, az};
  const int32_t* list = nullptr;
  int len = 0;
  if constexpr (LIST) {
    int beg;
    len = contact_list_span(csr_offset, robot, beg);
    list = csr_index + beg;
  }
  dynamics_step_contacts_robot<N, SLOTS, LIST, PlaneTable>(
      prog->ops, prog->n_ops, n_dof, inert, base_acc, q + row, qd + row, u + row, accel != 0, lim, qlo, qhi, caps, spheres, K, d_act,
      dt, substeps, qdd_out ? qdd_out + row : nullptr, tau_out ? tau_out + row : nullptr, stop_out ? stop_out + row : nullptr,
      contact_out ? contact_out + row : nullptr, lambda_out ? lambda_out + crow : nullptr, pair_out ? pair_out + crow : nullptr,
      status_out ? status_out + robot : nullptr, lds + threadIdx.x, kWave, list, len, PlaneTable{planes, P, F});
}

namespace {

template <int N, int S>
void launch(const rmp2_handle* h, float* q, float* qd, const float* u, int accel, const float* lim, const float* qlo,
            const float* qhi, const float* spheres, int K, const int32_t* csr_offset, const int32_t* csr_index, const float* planes,
            int P, float d_act, float dt, int substeps, float* qdd_out, float* tau_out, float* stop_out, float* contact_out,
            float* lambda_out, int32_t* pair_out, uint32_t* status_out, int R, hipStream_t s) {
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  hipLaunchKernelGGL((rmp2_dynamics_step_contacts_planes_kernel<N, S, RMP2_TU_LIST != 0>), grid, block, 0, s, h->d_prog_full,
                     h->d_inert, a[0], a[1], a[2], q, qd, u, accel, lim, qlo, qhi, h->d_contact_caps, spheres, K, csr_offset,
                     csr_index, planes, P, h->n_frames, d_act, dt, substeps, qdd_out, tau_out, stop_out, contact_out, lambda_out,
                     pair_out, status_out, R);
}

}  // namespace

// N = the handle's template size (2, or 9 for 3 .. 9 dofs), SLOTS = the unpruned program's save slots (0 .. 2)
#if RMP2_TU_LIST
void launch_dynamics_step_contacts_planes_lists(
#else
void launch_dynamics_step_contacts_planes_table(
#endif
    const rmp2_handle* h, float* q, float* qd, const float* u, int accel, const float* lim, const float* qlo, const float* qhi,
    const float* spheres, int K, const int32_t* csr_offset, const int32_t* csr_index, const float* planes, int P, float d_act,
    float dt, int substeps, float* qdd_out, float* tau_out, float* stop_out, float* contact_out, float* lambda_out,
    int32_t* pair_out, uint32_t* status_out, int R, hipStream_t s) {
#define RMP2_PLANES_ARGS h, q, qd, u, accel, lim, qlo, qhi, spheres, K, csr_offset, csr_index, planes, P, d_act, dt, substeps, \
                         qdd_out, tau_out, stop_out, contact_out, lambda_out, pair_out, status_out, R, s
  const int slots = h->n_slots_full;
  if (h->n_template == 2) {
    if (slots == 0) launch<2, 0>(RMP2_PLANES_ARGS);
    else if (slots == 1) launch<2, 1>(RMP2_PLANES_ARGS);
    else launch<2, 2>(RMP2_PLANES_ARGS);
  } else {
    if (slots == 0) launch<9, 0>(RMP2_PLANES_ARGS);
    else if (slots == 1) launch<9, 1>(RMP2_PLANES_ARGS);
    else launch<9, 2>(RMP2_PLANES_ARGS);
  }
#undef RMP2_PLANES_ARGS
}

}  // namespace rmp2

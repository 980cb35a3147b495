// rmp2_contacts_lists_tu.hip -- the instantiations of rmp2_dynamics_step_contacts_lists_kernel (rmp2_contacts.h) and their launcher.
// A translation unit of its own: a code object of its own, so that rmp2_hip.hip's device code -- rmp2_dynamics_step_contacts_kernel
// and every other kernel there -- stays byte for byte what it is without this entry point, placement in the code object included.
#include <cfloat>
#include <cmath>

#include "rmp2_host.h"
#include "rmp2_contacts.h"

namespace rmp2 {
namespace {

template <int N, int S>
void launch(const rmp2_handle* h, float* q, float* qd, const float* u, int accel, const float* lim, const float* qlo,
            const float* qhi, const float* spheres, int K, const int32_t* csr_offset, const int32_t* csr_index, float d_act, float dt,
            int substeps, float* qdd_out, float* tau_out, float* stop_out, float* contact_out, float* lambda_out, int32_t* pair_out,
            uint32_t* status_out, int R, hipStream_t s) {
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  hipLaunchKernelGGL((rmp2_dynamics_step_contacts_lists_kernel<N, S>), grid, block, 0, s, h->d_prog_full, h->d_inert, a[0], a[1],
                     a[2], q, qd, u, accel, lim, qlo, qhi, h->d_contact_caps, spheres, K, csr_offset, csr_index, d_act, dt,
                     substeps, qdd_out, tau_out, stop_out, contact_out, lambda_out, pair_out, status_out, R);
}

}  // namespace

// N = the handle's template size (2, or 9 for 3 .. 9 dofs), SLOTS = the unpruned program's save slots (0 .. 2)
void launch_dynamics_step_contacts_lists(const rmp2_handle* h, float* q, float* qd, const float* u, int accel, const float* lim,
                                         const float* qlo, const float* qhi, const float* spheres, int K, const int32_t* csr_offset,
                                         const int32_t* csr_index, float d_act, float dt, int substeps, float* qdd_out,
                                         float* tau_out, float* stop_out, float* contact_out, float* lambda_out, int32_t* pair_out,
                                         uint32_t* status_out, int R, hipStream_t s) {
#define RMP2_LISTS_ARGS h, q, qd, u, accel, lim, qlo, qhi, spheres, K, csr_offset, csr_index, d_act, dt, substeps, qdd_out, tau_out, \
                        stop_out, contact_out, lambda_out, pair_out, status_out, R, s
  const int slots = h->n_slots_full;
  if (h->n_template == 2) {
    if (slots == 0) launch<2, 0>(RMP2_LISTS_ARGS);
    else if (slots == 1) launch<2, 1>(RMP2_LISTS_ARGS);
    else launch<2, 2>(RMP2_LISTS_ARGS);
  } else {
    if (slots == 0) launch<9, 0>(RMP2_LISTS_ARGS);
    else if (slots == 1) launch<9, 1>(RMP2_LISTS_ARGS);
    else launch<9, 2>(RMP2_LISTS_ARGS);
  }
#undef RMP2_LISTS_ARGS
}

}  // namespace rmp2

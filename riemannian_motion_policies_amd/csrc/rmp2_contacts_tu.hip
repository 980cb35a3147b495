// rmp2_contacts_tu.hip -- the instantiations of rmp2_dynamics_step_contacts_kernel (rmp2_contacts.h) of one form and their launcher.
// Compiled four times, RMP2_TU_LIST = 0 (the shared sphere table) or 1 (per-robot lists over a pool) by RMP2_TU_PLANES = 0 or 1
// (half-spaces beside the spheres), each a code object of its own: a form's device code does not depend on the others' being there.
// With RMP2_TU_CAPSULES = 1 (and RMP2_TU_PLANES = 1) the unit holds the capsule forms instead -- planes and capsule obstacles on,
// rmp2_dynamics_step_contacts_capsules_kernel -- two more code objects, RMP2_TU_LIST = 0 and 1.  With RMP2_TU_SELF = 1 (and the
// other two) it holds the self forms -- the handle's self pairs on as well, rmp2_dynamics_step_contacts_self_kernel -- two more.
// With RMP2_TU_CYLINDERS = 1 (and the other three) it holds the cylinder forms -- the cylinder table on as well,
// rmp2_dynamics_step_contacts_cylinders_kernel -- two more.  With RMP2_TU_CYLINDER_LISTS = 1 (and the other four) it holds the
// cylinder-list forms -- every robot's own cylinder list over a pool, rmp2_dynamics_step_contacts_cylinder_lists_kernel -- two more.
#include <cfloat>
#include <cmath>

#include "rmp2_host.h"
#include "rmp2_contacts.h"

#if !defined(RMP2_TU_LIST) || !defined(RMP2_TU_PLANES)
#error "RMP2_TU_LIST and RMP2_TU_PLANES must each be 0 or 1"
#endif
#ifndef RMP2_TU_CAPSULES
#define RMP2_TU_CAPSULES 0
#endif
#if RMP2_TU_CAPSULES && !RMP2_TU_PLANES
#error "the capsule forms run with the planes on"
#endif
#ifndef RMP2_TU_SELF
#define RMP2_TU_SELF 0
#endif
#if RMP2_TU_SELF && !RMP2_TU_CAPSULES
#error "the self forms run with the planes and the capsules on"
#endif

#ifndef RMP2_TU_CYLINDERS
#define RMP2_TU_CYLINDERS 0
#endif
#if RMP2_TU_CYLINDERS && !RMP2_TU_SELF
#error "the cylinder forms run with the planes, the capsules and the self pairs on"
#endif

#ifndef RMP2_TU_CYLINDER_LISTS
#define RMP2_TU_CYLINDER_LISTS 0
#endif
#if RMP2_TU_CYLINDER_LISTS && !RMP2_TU_CYLINDERS
#error "the cylinder-list forms are cylinder forms"
#endif

namespace rmp2 {

#if RMP2_TU_CYLINDER_LISTS
#if RMP2_TU_LIST
RMP2_DECL_CONTACTS_CYLINDER_LISTS(launch_contacts_lists_cylinder_lists) {
#else
RMP2_DECL_CONTACTS_CYLINDER_LISTS(launch_contacts_table_cylinder_lists) {
#endif
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  // the handle's pair tables, where the call asks for them (self_pairs); else the kernel reads none of them
  const int n_ops = (int)h->full_op_frame.size(), n_self = self_pairs ? h->contact_self_n : 0;
  const int32_t* slot = n_self ? h->d_contact_self : nullptr;
  const int32_t* begin = n_self ? slot + n_ops : nullptr;
  const int32_t* rec = n_self ? begin + n_ops + 1 : nullptr;
  auto launch = [&](auto N) {
    with_slots(h->n_slots_full, [&](auto S) {
      hipLaunchKernelGGL((rmp2_dynamics_step_contacts_cylinder_lists_kernel<N, S, RMP2_TU_LIST != 0>), grid, block, 0, s,
                         h->d_prog_full, h->d_inert, a[0], a[1], a[2], q, qd, u, accel, lim, qlo, qhi, h->d_contact_caps, spheres, K,
                         csr_offset, csr_index, planes, P, capsules, C, slot, begin, rec, n_self, cylinders, Y, cyl_offset, cyl_index,
                         h->n_frames, d_act, dt, substeps, qdd_out, tau_out, stop_out, contact_out, lambda_out, pair_out, status_out,
                         R);
    });
  };
  if (h->n_template == 2) launch(std::integral_constant<int, 2>());
  else launch(std::integral_constant<int, 9>());
}
#elif RMP2_TU_CYLINDERS
#if RMP2_TU_LIST
RMP2_DECL_CONTACTS_CYLINDERS(launch_contacts_lists_cylinders) {
#else
RMP2_DECL_CONTACTS_CYLINDERS(launch_contacts_table_cylinders) {
#endif
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  // the handle's pair tables, where the call asks for them (self_pairs); else the kernel reads none of them
  const int n_ops = (int)h->full_op_frame.size(), n_self = self_pairs ? h->contact_self_n : 0;
  const int32_t* slot = n_self ? h->d_contact_self : nullptr;
  const int32_t* begin = n_self ? slot + n_ops : nullptr;
  const int32_t* rec = n_self ? begin + n_ops + 1 : nullptr;
  auto launch = [&](auto N) {
    with_slots(h->n_slots_full, [&](auto S) {
      hipLaunchKernelGGL((rmp2_dynamics_step_contacts_cylinders_kernel<N, S, RMP2_TU_LIST != 0>), grid, block, 0, s, h->d_prog_full,
                         h->d_inert, a[0], a[1], a[2], q, qd, u, accel, lim, qlo, qhi, h->d_contact_caps, spheres, K, csr_offset,
                         csr_index, planes, P, capsules, C, slot, begin, rec, n_self, cylinders, Y, h->n_frames, d_act, dt, substeps,
                         qdd_out, tau_out, stop_out, contact_out, lambda_out, pair_out, status_out, R);
    });
  };
  if (h->n_template == 2) launch(std::integral_constant<int, 2>());
  else launch(std::integral_constant<int, 9>());
}
#elif RMP2_TU_SELF
#if RMP2_TU_LIST
RMP2_DECL_CONTACTS_CAPSULES(launch_contacts_lists_self) {
#else
RMP2_DECL_CONTACTS_CAPSULES(launch_contacts_table_self) {
#endif
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  // the handle's pair tables (rmp2_set_contact_self_pairs); without pairs the kernel reads none of them
  const int n_ops = (int)h->full_op_frame.size(), n_self = h->contact_self_n;
  const int32_t* slot = n_self ? h->d_contact_self : nullptr;
  const int32_t* begin = n_self ? slot + n_ops : nullptr;
  const int32_t* rec = n_self ? begin + n_ops + 1 : nullptr;
  auto launch = [&](auto N) {
    with_slots(h->n_slots_full, [&](auto S) {
      hipLaunchKernelGGL((rmp2_dynamics_step_contacts_self_kernel<N, S, RMP2_TU_LIST != 0>), grid, block, 0, s, h->d_prog_full,
                         h->d_inert, a[0], a[1], a[2], q, qd, u, accel, lim, qlo, qhi, h->d_contact_caps, spheres, K, csr_offset,
                         csr_index, planes, P, capsules, C, slot, begin, rec, n_self, h->n_frames, d_act, dt, substeps, qdd_out,
                         tau_out, stop_out, contact_out, lambda_out, pair_out, status_out, R);
    });
  };
  if (h->n_template == 2) launch(std::integral_constant<int, 2>());
  else launch(std::integral_constant<int, 9>());
}
#elif RMP2_TU_CAPSULES
#if RMP2_TU_LIST
RMP2_DECL_CONTACTS_CAPSULES(launch_contacts_lists_capsules) {
#else
RMP2_DECL_CONTACTS_CAPSULES(launch_contacts_table_capsules) {
#endif
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  auto launch = [&](auto N) {
    with_slots(h->n_slots_full, [&](auto S) {
      hipLaunchKernelGGL((rmp2_dynamics_step_contacts_capsules_kernel<N, S, RMP2_TU_LIST != 0>), grid, block, 0, s, h->d_prog_full,
                         h->d_inert, a[0], a[1], a[2], q, qd, u, accel, lim, qlo, qhi, h->d_contact_caps, spheres, K, csr_offset,
                         csr_index, planes, P, capsules, C, h->n_frames, d_act, dt, substeps, qdd_out, tau_out, stop_out, contact_out,
                         lambda_out, pair_out, status_out, R);
    });
  };
  if (h->n_template == 2) launch(std::integral_constant<int, 2>());
  else launch(std::integral_constant<int, 9>());
}
#else
#if RMP2_TU_LIST && RMP2_TU_PLANES
RMP2_DECL_CONTACTS(launch_contacts_lists_planes) {
#elif RMP2_TU_LIST
RMP2_DECL_CONTACTS(launch_contacts_lists) {
#elif RMP2_TU_PLANES
RMP2_DECL_CONTACTS(launch_contacts_table_planes) {
#else
RMP2_DECL_CONTACTS(launch_contacts_table) {
#endif
  const dim3 grid((R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  // N = the handle's template size (2, or 9 for 3 .. 9 dofs), SLOTS = the unpruned program's save slots (0 .. 2)
  auto launch = [&](auto N) {
    with_slots(h->n_slots_full, [&](auto S) {
      hipLaunchKernelGGL((rmp2_dynamics_step_contacts_kernel<N, S, RMP2_TU_LIST != 0, RMP2_TU_PLANES != 0>), grid, block, 0, s,
                         h->d_prog_full, h->d_inert, a[0], a[1], a[2], q, qd, u, accel, lim, qlo, qhi, h->d_contact_caps, spheres, K,
                         csr_offset, csr_index, planes, P, h->n_frames, d_act, dt, substeps, qdd_out, tau_out, stop_out, contact_out,
                         lambda_out, pair_out, status_out, R);
    });
  };
  if (h->n_template == 2) launch(std::integral_constant<int, 2>());
  else launch(std::integral_constant<int, 9>());
}
#endif

}  // namespace rmp2

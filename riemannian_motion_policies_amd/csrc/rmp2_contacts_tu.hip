// rmp2_contacts_tu.hip -- the instantiations of ONE contact kernel of rmp2_contacts.h and their launcher.  Compiled twelve times,
// each a code object of its own (a form's device code does not depend on the others' being there): RMP2_TU_LIST = 0 (the shared
// sphere table) or 1 (per-robot sphere lists over a pool) by the form, which the other flags select cumulatively --
// RMP2_TU_PLANES = 0 / 1 (rmp2_dynamics_step_contacts_kernel without / with half-spaces), then with it RMP2_TU_CAPSULES = 1
// (..._capsules_kernel), with both RMP2_TU_SELF = 1 (..._self_kernel), with those RMP2_TU_CYLINDERS = 1 (..._cylinders_kernel), with
// all of them RMP2_TU_CYLINDER_LISTS = 1 (..._cylinder_lists_kernel).  The launcher is one body; what differs per form -- the
// launcher's name, the kernel, the tail of its argument list and the rule for the self tables -- is the macros below.
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

// RMP2_TU_NAME: the unit's launcher, of RMP2_TU_LAUNCHER's two by RMP2_TU_LIST.  RMP2_TU_KERNEL (N, S): its kernel.
// RMP2_TU_FORM_ARGS: the kernel's arguments between csr_index and F (RMP2_TU_SELF_ARGS: those of the self form, which the cylinder
// forms extend).  RMP2_TU_SELF_TABLES: whether the handle's pair tables are passed -- the self form always, the cylinder forms where
// the call asks for them (self_pairs).
#if RMP2_TU_LIST
#define RMP2_TU_LAUNCHER(table, lists) lists
#else
#define RMP2_TU_LAUNCHER(table, lists) table
#endif
#if RMP2_TU_SELF
#define RMP2_TU_SELF_ARGS c.planes, c.P, c.capsules, c.C, slot, begin, rec, n_self
#endif
#if RMP2_TU_CYLINDER_LISTS
#define RMP2_TU_NAME RMP2_TU_LAUNCHER(launch_contacts_table_cylinder_lists, launch_contacts_lists_cylinder_lists)
#define RMP2_TU_KERNEL(N, S) rmp2_dynamics_step_contacts_cylinder_lists_kernel<N, S, RMP2_TU_LIST != 0>
#define RMP2_TU_FORM_ARGS RMP2_TU_SELF_ARGS, c.cylinders, c.Y, c.cyl_offset, c.cyl_index
#define RMP2_TU_SELF_TABLES c.self_pairs
#elif RMP2_TU_CYLINDERS
#define RMP2_TU_NAME RMP2_TU_LAUNCHER(launch_contacts_table_cylinders, launch_contacts_lists_cylinders)
#define RMP2_TU_KERNEL(N, S) rmp2_dynamics_step_contacts_cylinders_kernel<N, S, RMP2_TU_LIST != 0>
#define RMP2_TU_FORM_ARGS RMP2_TU_SELF_ARGS, c.cylinders, c.Y
#define RMP2_TU_SELF_TABLES c.self_pairs
#elif RMP2_TU_SELF
#define RMP2_TU_NAME RMP2_TU_LAUNCHER(launch_contacts_table_self, launch_contacts_lists_self)
#define RMP2_TU_KERNEL(N, S) rmp2_dynamics_step_contacts_self_kernel<N, S, RMP2_TU_LIST != 0>
#define RMP2_TU_FORM_ARGS RMP2_TU_SELF_ARGS
#define RMP2_TU_SELF_TABLES true
#elif RMP2_TU_CAPSULES
#define RMP2_TU_NAME RMP2_TU_LAUNCHER(launch_contacts_table_capsules, launch_contacts_lists_capsules)
#define RMP2_TU_KERNEL(N, S) rmp2_dynamics_step_contacts_capsules_kernel<N, S, RMP2_TU_LIST != 0>
#define RMP2_TU_FORM_ARGS c.planes, c.P, c.capsules, c.C
#define RMP2_TU_SELF_TABLES false
#else
#if RMP2_TU_PLANES
#define RMP2_TU_NAME RMP2_TU_LAUNCHER(launch_contacts_table_planes, launch_contacts_lists_planes)
#else
#define RMP2_TU_NAME RMP2_TU_LAUNCHER(launch_contacts_table, launch_contacts_lists)
#endif
#define RMP2_TU_KERNEL(N, S) rmp2_dynamics_step_contacts_kernel<N, S, RMP2_TU_LIST != 0, RMP2_TU_PLANES != 0>
#define RMP2_TU_FORM_ARGS c.planes, c.P
#define RMP2_TU_SELF_TABLES false
#endif

namespace rmp2 {

void RMP2_TU_NAME(const rmp2_handle* h, const ContactCall& c, hipStream_t s) {
  const dim3 grid((c.R + kWave - 1) / kWave), block(kWave);
  const float* a = h->base_acc;
  // the handle's pair tables (rmp2_set_contact_self_pairs); without pairs, or where they are not passed, the kernel reads none
  const int n_ops = (int)h->full_op_frame.size(), n_self = RMP2_TU_SELF_TABLES ? h->contact_self_n : 0;
  [[maybe_unused]] const int32_t* slot = n_self ? h->d_contact_self : nullptr;
  [[maybe_unused]] const int32_t* begin = n_self ? slot + n_ops : nullptr;
  [[maybe_unused]] const int32_t* rec = n_self ? begin + n_ops + 1 : nullptr;
  // N = the handle's template size (2, or 9 for 3 .. 9 dofs), SLOTS = the unpruned program's save slots (0 .. 2)
  auto launch = [&](auto N) {
    with_slots(h->n_slots_full, [&](auto S) {
      hipLaunchKernelGGL((RMP2_TU_KERNEL(N, S)), grid, block, 0, s, h->d_prog_full, h->d_inert, a[0], a[1], a[2], c.q, c.qd, c.u, c.accel, c.lim,
                         c.qlo, c.qhi, h->d_contact_caps, c.spheres, c.K, c.csr_offset, c.csr_index, RMP2_TU_FORM_ARGS, h->n_frames, c.d_act,
                         c.dt, c.substeps, c.qdd_out, c.tau_out, c.stop_out, c.contact_out, c.lambda_out, c.pair_out, c.status_out, c.R);
    });
  };
  if (h->n_template == 2) launch(std::integral_constant<int, 2>());
  else launch(std::integral_constant<int, 9>());
}

}  // namespace rmp2

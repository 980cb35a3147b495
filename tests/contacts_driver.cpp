// Host driver of rmp2_contacts.h for every contact host test (tests/test_contacts*_host.py, tests/test_contact_*_host.py): no GPU,
// the device routine's own code on the CPU (dynamics_step_contacts_robot<N, SLOTS, LIST, Pl, Cp, Sp, Cy>, what the kernels call),
// the per-lane storage in a local array (stride 1), with the template sizes the library picks.  usage: driver IN OUT FORM.
//
// IN (native byte order) is cumulative, each writer appending to the one before; a section that FORM needs must be there, later
// ones may be and are read and checked all the same:
//   tests/contacts_reference.py write_driver_input: the input of tests/forward_dynamics_driver.cpp in mode 2, int32 has_limits, float
//     lower[n_dof], upper[n_dof], float caps[F][8], int32 K, float d_act, float spheres[K][4], int32 has_lists, [int32
//     offset[n_states + 1], int32 n_index, int32 index[n_index]] when has_lists (the table is then the POOL, K <=
//     RMP2_MAX_CONTACT_POOL), int32 has_planes, [int32 P, float planes[P][4]] when has_planes;
//   tests/contact_capsules_reference.py (the plane section present): int32 C, float capsules[C][8];
//   tests/contact_self_reference.py: int32 n_pairs and, where n_pairs > 0, int32 slot[n_ops], begin[n_ops + 1], rec[n_pairs][4];
//   tests/contact_cylinders_reference.py: int32 Y, float cylinders[Y][8], int32 self_pairs (the call's flag);
//   tests/contact_cylinder_lists_scene.py: int32 cyl_offset[n_states + 1], int32 n_index, int32 cyl_index[n_index].
// FORM picks the instantiation as the library's entry point picks the kernel; the sphere form (LIST) follows has_lists in all:
//   contacts        Pl = NoPlanes without a plane section, PlaneTable with one (P = 0 too); contact_words(N) words per lane
//   capsules        + CapsuleTable (C = 0 too); contact_words(N)
//   self            + SelfPairs, the file's pair tables (none: null, n = 0); contact_self_words(N), as the two below
//   cylinders       + CylinderTable (Y <= RMP2_MAX_OBSTACLE_CYLINDERS); with the flag 0 the pair tables are not handed on, as the
//                   library's launcher does it.  On a file with cylinder lists: the pool as the shared table, the lists ignored
//   cylinder_lists  CylinderList in its place (Y <= RMP2_MAX_CYLINDER_POOL)
// All forms are compiled into this one program, so that their bits can be compared.  Output (OUT): float q, qd, qdd, tau, stop,
// contact [n_states][n_dof] each, float lambda[n_states][8], int32 pair[n_states][8], uint32 status[n_states].  Every table is
// allocated at exactly its size, so that a sanitizer build sees any read past it or through a bad entry; a self or cylinder table
// without records is null.  Built with -DRMP2_CYLINDER_NO_CULL the cylinder trip runs without the cull in front of the bisection.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "rmp2_contacts.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static bool at_end(FILE* f) {
  const int ch = fgetc(f);
  if (ch != EOF) ungetc(ch, f);
  return ch == EOF;
}

enum Form { kSpheres, kPlanes, kCapsules, kSelf, kCylinders, kCylinderLists };

struct Job {
  std::vector<rmp2::DevOp> ops;
  int n, B, drive, substeps, K;
  float dt, d_act;
  std::vector<float> inert, acc, lim, lo, hi, caps, q, qd, u, qdd, tau, stop, contact, lambda;
  std::unique_ptr<float[]> spheres;     // exactly [K][4]
  std::unique_ptr<int32_t[]> index;     // exactly [n_index]
  std::unique_ptr<float[]> planes;      // exactly [P][4]
  std::unique_ptr<float[]> capsules;    // exactly [C][8]
  std::unique_ptr<int32_t[]> self_slot, self_begin, self_rec;   // exactly [n_ops], [n_ops + 1], [n_self][4]
  std::unique_ptr<float[]> cylinders;   // exactly [Y][8]
  std::unique_ptr<int32_t[]> cyl_index;  // exactly [n_cyl_index]
  int P = 0, C = 0, n_self = 0, Y = 0, flag = 1;
  std::vector<int32_t> pair, offset, cyl_offset;
  std::vector<uint32_t> status;
  bool has_lim, has_limits;
};

template <int N, int SLOTS, bool LIST, Form FORM>
static void run(Job& j) {
  using Pl = std::conditional_t<FORM >= kPlanes, rmp2::PlaneTable, rmp2::NoPlanes>;
  using Cp = std::conditional_t<FORM >= kCapsules, rmp2::CapsuleTable, rmp2::NoCapsules>;
  using Sp = std::conditional_t<FORM >= kSelf, rmp2::SelfPairs, rmp2::NoSelfPairs>;
  using Cy = std::conditional_t<FORM == kCylinderLists, rmp2::CylinderList,
                                std::conditional_t<FORM == kCylinders, rmp2::CylinderTable, rmp2::NoCylinders>>;
  const int n = j.n, F = (int)j.ops.size();
  std::vector<float> lds(FORM >= kSelf ? rmp2::contact_self_words(N) : rmp2::contact_words(N));
  for (int b = 0; b < j.B; ++b) {
    const size_t o = (size_t)b * n, c = (size_t)b * rmp2::kMaxContacts;
    int beg = 0, len = 0;
    if (LIST) len = rmp2::contact_list_span(j.offset.data(), b, beg);
    Pl pl{};
    Cp oc{};
    Sp sp{};
    Cy cy{};
    if constexpr (Pl::kOn) pl = {j.planes.get(), j.P, F};
    if constexpr (Cp::kOn) oc = {j.capsules.get(), j.C, F, j.P};
    if constexpr (Sp::kOn) {
      const int n_self = FORM == kSelf || j.flag ? j.n_self : 0;
      sp = {n_self ? j.self_slot.get() : nullptr, n_self ? j.self_begin.get() : nullptr, n_self ? j.self_rec.get() : nullptr, n_self,
            F, nullptr};
    }
    if constexpr (FORM == kCylinderLists) {
      int cbeg = 0;
      const int clen = rmp2::contact_list_span(j.cyl_offset.data(), b, cbeg);
      cy = rmp2::CylinderList{j.cylinders.get(), j.Y, j.cyl_index.get() + cbeg, clen, F, j.P, j.C};
    } else if constexpr (FORM == kCylinders) {
      cy = {j.cylinders.get(), j.Y, F, j.P, j.C};
    }
    rmp2::dynamics_step_contacts_robot<N, SLOTS, LIST, Pl, Cp, Sp, Cy>(
        j.ops.data(), F, n, j.inert.data(), j.acc.data(), j.q.data() + o, j.qd.data() + o, j.u.data() + o,
        j.drive == RMP2_DRIVE_ACCEL, j.has_lim ? j.lim.data() : nullptr, j.has_limits ? j.lo.data() : nullptr,
        j.has_limits ? j.hi.data() : nullptr, j.caps.data(), j.spheres.get(), j.K, j.d_act, j.dt, j.substeps,
        j.qdd.data() + o, j.tau.data() + o, j.stop.data() + o, j.contact.data() + o, j.lambda.data() + c, j.pair.data() + c,
        j.status.data() + b, lds.data(), 1, LIST ? j.index.get() + beg : nullptr, len, pl, oc, sp, cy);
  }
}

template <int N, int SLOTS, bool LIST>
static void run_form(Form form, Job& j) {
  switch (form) {
    case kSpheres: return run<N, SLOTS, LIST, kSpheres>(j);
    case kPlanes: return run<N, SLOTS, LIST, kPlanes>(j);
    case kCapsules: return run<N, SLOTS, LIST, kCapsules>(j);
    case kSelf: return run<N, SLOTS, LIST, kSelf>(j);
    case kCylinders: return run<N, SLOTS, LIST, kCylinders>(j);
    case kCylinderLists: return run<N, SLOTS, LIST, kCylinderLists>(j);
  }
}

template <int N>
static void run_n(int slots, bool lists, Form form, Job& j) {
  if (slots == 0) lists ? run_form<N, 0, true>(form, j) : run_form<N, 0, false>(form, j);
  else if (slots == 1) lists ? run_form<N, 1, true>(form, j) : run_form<N, 1, false>(form, j);
  else lists ? run_form<N, 2, true>(form, j) : run_form<N, 2, false>(form, j);
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  static const char* const kNames[] = {"contacts", "capsules", "self", "cylinders", "cylinder_lists"};
  int named = 0;
  while (named < 5 && std::strcmp(argv[3], kNames[named])) ++named;
  if (named == 5) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hdr[9];
  Job j;
  if (!rd(f, hdr, 9) || !rd(f, &j.dt, 1)) return 4;
  const int n_ops = hdr[0], F = hdr[1], n = hdr[2], slots = hdr[3], B = hdr[4];
  j.n = n, j.B = B, j.drive = hdr[6], j.substeps = hdr[7], j.has_lim = hdr[8] != 0;
  if (n_ops < 1 || n_ops > RMP2_MAX_FRAMES || F != n_ops || n < 1 || n > 9 || slots < 0 || slots > 2 || B < 0 || hdr[5] != 2 ||
      j.substeps < 1)
    return 5;
  j.ops.resize(n_ops);
  for (auto& op : j.ops) {
    std::memset(&op, 0, sizeof(op));
    int32_t v[5];
    uint32_t mask;
    if (!rd(f, v, 5) || !rd(f, &mask, 1) || !rd(f, op.axis, 3) || !rd(f, op.Tc, 12)) return 6;
    op.frame = v[0], op.restore = v[1], op.save = v[2], op.jtype = v[3], op.qidx = v[4], op.anc_mask = mask;
    if (op.frame < 0 || op.frame >= F || op.qidx >= n || op.restore >= slots || op.save >= slots) return 7;
  }
  j.inert.resize((size_t)F * rmp2::kInertialFloats), j.acc.resize(3), j.lim.resize(n), j.lo.resize(n), j.hi.resize(n);
  j.caps.resize((size_t)F * 8);
  j.q.resize((size_t)B * n), j.qd.resize(j.q.size()), j.u.resize(j.q.size()), j.qdd.resize(j.q.size()), j.tau.resize(j.q.size());
  j.stop.resize(j.q.size()), j.contact.resize(j.q.size()), j.status.resize(B);
  j.lambda.resize((size_t)B * rmp2::kMaxContacts), j.pair.resize(j.lambda.size());
  int32_t has_limits = 0, K = 0;
  if (!rd(f, j.inert.data(), j.inert.size()) || !rd(f, j.acc.data(), 3) || !rd(f, j.lim.data(), j.lim.size()) ||
      !rd(f, j.q.data(), j.q.size()) || !rd(f, j.qd.data(), j.qd.size()) || !rd(f, j.u.data(), j.u.size()) ||
      !rd(f, &has_limits, 1) || !rd(f, j.lo.data(), j.lo.size()) || !rd(f, j.hi.data(), j.hi.size()) ||
      !rd(f, j.caps.data(), j.caps.size()) || !rd(f, &K, 1) || !rd(f, &j.d_act, 1))
    return 8;
  j.K = K, j.has_limits = has_limits != 0;
  if (K < 0 || K > RMP2_MAX_CONTACT_POOL) return 5;
  j.spheres.reset(new float[(size_t)K * 4]);
  int32_t has_lists = 0, n_index = 0, has_planes = 0, P = 0;
  if (!rd(f, j.spheres.get(), (size_t)K * 4) || !rd(f, &has_lists, 1)) return 8;
  if (!has_lists && K > RMP2_MAX_CONTACT_SPHERES) return 5;
  if (has_lists) {
    j.offset.resize((size_t)B + 1);
    if (!rd(f, j.offset.data(), j.offset.size()) || !rd(f, &n_index, 1) || n_index < 0) return 8;
    j.index.reset(new int32_t[n_index]);
    if (!rd(f, j.index.get(), (size_t)n_index)) return 8;
  }
  if (!rd(f, &has_planes, 1)) return 8;
  // the form by what was asked for; the sections up to it must be there (`have` counts them in Form's order)
  Form form = named == 0 ? (has_planes ? kPlanes : kSpheres) : (Form)(named + 1);
  if (form >= kCapsules && !has_planes) return 5;
  Form have = kSpheres;
  if (has_planes) {
    if (!rd(f, &P, 1) || P < 0 || P > RMP2_MAX_CONTACT_PLANES) return 8;
    j.P = P;
    j.planes.reset(new float[(size_t)P * 4]);
    if (!rd(f, j.planes.get(), (size_t)P * 4)) return 8;
    have = kPlanes;
  }
  if (has_planes && !at_end(f)) {
    int32_t C = 0;
    if (!rd(f, &C, 1) || C < 0 || C > RMP2_MAX_OBSTACLE_CAPSULES) return 8;
    j.C = C;
    j.capsules.reset(new float[(size_t)C * 8]);
    if (!rd(f, j.capsules.get(), (size_t)C * 8)) return 8;
    have = kCapsules;
  }
  if (have == kCapsules && !at_end(f)) {
    int32_t n_self = 0;
    if (!rd(f, &n_self, 1) || n_self < 0 || n_self > RMP2_MAX_FRAMES * (RMP2_MAX_FRAMES - 1) / 2) return 8;
    j.n_self = n_self;
    if (n_self > 0) {
      j.self_slot.reset(new int32_t[n_ops]), j.self_begin.reset(new int32_t[n_ops + 1]), j.self_rec.reset(new int32_t[(size_t)n_self * 4]);
      if (!rd(f, j.self_slot.get(), (size_t)n_ops) || !rd(f, j.self_begin.get(), (size_t)n_ops + 1) ||
          !rd(f, j.self_rec.get(), (size_t)n_self * 4))
        return 8;
      // what rmp2_set_contact_self_pairs guarantees: slots within the kernel's storage, the records within the tables
      if (j.self_begin[0] != 0 || j.self_begin[n_ops] != n_self) return 5;
      for (int k = 0; k < n_ops; ++k)
        if (j.self_slot[k] < -1 || j.self_slot[k] >= RMP2_MAX_CONTACT_SELF_FRAMES || j.self_begin[k + 1] < j.self_begin[k]) return 5;
      for (int p = 0; p < n_self; ++p)
        if (j.self_rec[4 * p] < 0 || j.self_rec[4 * p] >= RMP2_MAX_CONTACT_SELF_FRAMES || j.self_rec[4 * p + 1] < 0 ||
            j.self_rec[4 * p + 1] >= F)
          return 5;
    }
    have = kSelf;
  }
  if (have == kSelf && !at_end(f)) {
    int32_t Y = 0, flag = 0;
    if (!rd(f, &Y, 1) || Y < 0 || Y > (form == kCylinders ? RMP2_MAX_OBSTACLE_CYLINDERS : RMP2_MAX_CYLINDER_POOL)) return 8;
    j.Y = Y;
    if (Y > 0) j.cylinders.reset(new float[(size_t)Y * 8]);
    if (!rd(f, j.cylinders.get(), (size_t)Y * 8) || !rd(f, &flag, 1) || (flag != 0 && flag != 1)) return 8;
    j.flag = flag;
    have = kCylinders;
  }
  if (have == kCylinders && !at_end(f)) {
    int32_t n_cyl_index = 0;
    j.cyl_offset.resize((size_t)B + 1);
    if (!rd(f, j.cyl_offset.data(), j.cyl_offset.size()) || !rd(f, &n_cyl_index, 1) || n_cyl_index < 0) return 8;
    j.cyl_index.reset(new int32_t[n_cyl_index]);
    if (!rd(f, j.cyl_index.get(), (size_t)n_cyl_index)) return 8;
    have = kCylinderLists;
  }
  if (have < form || !at_end(f)) return 8;
  fclose(f);
  if (n <= 2) run_n<2>(slots, has_lists != 0, form, j);
  else run_n<9>(slots, has_lists != 0, form, j);
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 9;
  for (const auto* x : {&j.q, &j.qd, &j.qdd, &j.tau, &j.stop, &j.contact, &j.lambda}) fwrite(x->data(), sizeof(float), x->size(), g);
  fwrite(j.pair.data(), sizeof(int32_t), j.pair.size(), g);
  fwrite(j.status.data(), sizeof(uint32_t), j.status.size(), g);
  return fclose(g) == 0 ? 0 : 10;
}

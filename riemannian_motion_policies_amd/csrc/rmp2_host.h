// rmp2_host.h -- host-side pieces shared by the translation units of librmp2_hip.so: the engine handle, the step
// launch macro, and the launcher entry points of the per-mapping translation units (rmp2_quad_tu.hip, rmp2_hex_tu.hip).
// The kernels are templates in headers; each mapping is INSTANTIATED in its own translation unit so that the library
// builds in parallel (the quad kernel alone has ~70 instantiations) and a change to one mapping recompiles only it.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "rmp2_device.h"
#include "rmp2_solve.h"
#include "rmp2_quad.h"
#include "rmp2_hex.h"

struct rmp2_handle {
  int device = 0;
  int n_dof = 0, n_frames = 0, n_slots = 0, n_leaves = 0, goal_floats = 0;
  int n_slots_full = 0;  // slots of the unpruned program (FK / differentiate entry points)
  int n_ops_step = 0;    // frames the control-step kernels visit (pruned + folded program)
  rmp2::DevProgram* d_prog_full = nullptr;
  int n_template = 0;  // N of the kernel instantiation
  bool has_distance = false;
  bool has_point = false;  // attached-point leaves (CollisionAvoidance): hex and lane-per-robot kernels
  int n_id_leaves = 0;
  bool id_structured = false;  // every identity leaf is m * I or the velocity cap: the quad kernel's structured identity-leaf loop
  int n_leaf_ops = 0;
  uint32_t rev_mask = 0;
  float cull_c0 = 0.f;  // max over the distance leaves of (metric_modulation_radius + margin): beyond it a pair is culled
  uint32_t dof_ops[3] = {0u, 0u, 0u};  // op that owns each dof (quad kernel: Jacobian columns come from the frame slots)
  bool strict = false;  // solve_mode == RMP2_SOLVE_PINV
  bool strict_certify = true;  // RMP2_STRICT_CERTIFY=0: the Jacobi pseudo-inverse on every robot (A/B)
  bool link_rows_ok = false;   // <= 1 distance leaf per frame: link geometry may take the lean builds (segments formed in the walk)
  bool explicit_glds = false;  // RMP2_EXPLICIT_GLDS=1: explicit pairs streamed half a leaf ahead by LDS-DMA (measured: no gain)
  int stream_stagger = 0;    // RMP2_STREAM_STAGGER=n: start offset between the four waves of a SIMD in the streamed explicit-pair step, units of 3.4 us
  int explicit_stream = -1;  // RMP2_EXPLICIT_STREAM=0|1: never / at any throughput grid take the streamed explicit-pair step (A/B; -1: by grid size)
  bool likely_singular = false;  // no positive-definite identity leaf in the set
  int kernel_choice = 0;  // 0 auto, 1 lane-per-robot, 2 quad-per-robot, 3 hex (env RMP2_KERNEL=lane|quad|hex, A/B only)
  int hex_levels = 0;
  int hex_waves = 4;  // waves per block of the hex kernel (env RMP2_HEX_WAVES=1|4, A/B only)
  int quad_minw = 0;  // register cap of the throughput quad build: 0 = by fleet size (2, 3 or 4 waves per SIMD, launch_quad);
                      // env RMP2_QUAD_MINW=2|3|4 pins it (A/B only)
  int n_simd = 1024;  // SIMDs of the device (4 per CU)
  void* step_fence = nullptr;  // rmp2_set_step_fence: completion fence of the step launches (nullptr: none)
  bool symmetric = false;      // no leaf with a non-symmetric metric (JointLimitAvoidance, quirk Q2) in the set
  int prio_tail = -1;          // env RMP2_PRIO_TAIL=0..3 pins the priority of the phases after the frame loop (A/B only)
  bool quad_latency_set = false;   // RMP2_QUAD_LATENCY_BLOCKS given (tuning builds)
  int quad_latency_blocks = 0;     // grids up to this many waves take the latency build: none since round 5 (tuning builds: env RMP2_QUAD_LATENCY_BLOCKS)
  int n_fk_leaves = 0;
  int hex_is_chain = 0;
  void* d_hex_blob = nullptr;  // the staged program of the hex kernel, laid out exactly as it sits in LDS
  int hex_blob16 = 0;          // its size in 16-byte units
  std::vector<int> distance_leaves;
  rmp2::DevProgram* d_prog = nullptr;
  int32_t* d_pair_begin = nullptr;
  int32_t h_pair_begin[RMP2_MAX_LEAVES + 1];
  bool pair_begin_valid = false;
  float* d_scratch = nullptr;  // rmp2_differentiate scratch
  size_t scratch_robots = 0;
  // The stage buffer of a staged step (rmp2_hip.hip step_impl: link geometry beyond the fused limits, self collision or link hulls),
  // whose pairs the explicit-pair step then reads.  At most one stage runs per step, so the routes share it; its layout and size
  // depend on the route in use.  It grows to the largest need seen (a graph captured on a staged step stays valid until it grows).
  float* d_stage = nullptr;
  size_t stage_floats = 0;
  double* d_system = nullptr;  // [robots][n_dof * (n_dof + 1)] combined metric and force between the quad step and rmp2_pinv_kernel
  size_t system_robots = 0;
  // self collision (rmp2_set_self_collision): off while self_n_pairs == 0
  int self_n_pairs = 0;
  int self_n_b = 0;                     // B slots of the list
  std::vector<int> pair_leaves;         // descriptor indices of the FK_DISTANCE / FK_POINT leaves, descriptor order (the ordinals)
  std::vector<int> pair_leaf_frame;     // their frames
  std::vector<char> pair_leaf_point;    // 1: FK_POINT
  std::vector<int> self_counts;         // S_l per ordinal
  void* d_self = nullptr;               // SelfProg (rmp2_hip.hip)
  // Convex hulls: one HullProg and one set of vertex / plane arrays, for whichever hull geometry is on -- link hulls
  // (rmp2_set_link_hulls) or hull self pairs (rmp2_set_self_collision_hulls), which exclude each other.  With hull self pairs the
  // HullProg covers the pair leaves' hulls (the obstacle half); the arrays hold those first, in ordinal order, then the other entries.
  int hull_n = 0;                       // link hulls: off while 0
  void* d_hull = nullptr;               // HullProg (rmp2_hip.hip)
  float4* d_hull_verts = nullptr;       // (x, y, z, -) per vertex, hulls back to back
  float4* d_hull_planes = nullptr;      // (n, d) per face
  size_t hull_verts_cap = 0, hull_planes_cap = 0;
  // hull self pairs (rmp2_set_self_collision_hulls): the self-collision list above, on hulls while self_hulls is set
  bool self_hulls = false;
  bool shull_leaf_empty = false;        // some pair leaf has no hull: no obstacle pairs on such a handle
  int shull_slots = 0;                  // frame slots of the stage's LDS
  void* d_shull = nullptr;              // SelfHullProg (rmp2_hip.hip)
  // inverse dynamics (rmp2_set_inertials): off while inert_n == 0
  int inert_n = 0;
  float* d_inert = nullptr;             // [n_frames][10] inertial records
  // obstacle contacts (rmp2_set_contact_capsules): off while contact_n == 0
  int contact_n = 0;
  float* d_contact_caps = nullptr;      // [n_frames][8] link capsules in frame coordinates
  float base_acc[3] = {0.f, 0.f, 9.81f};  // -g
  // self contacts (rmp2_set_contact_self_pairs): off while contact_self_n == 0
  int contact_self_n = 0;
  int32_t* d_contact_self = nullptr;    // SelfPairs' tables back to back: slot [n_ops], begin [n_ops + 1], rec [contact_self_n][4]
  std::vector<int32_t> full_op_frame;   // the unpruned program's frames in op order, and the dofs that move each
  std::vector<uint32_t> full_op_anc;
  mutable bool quad_skip_resolve = false;  // set around that quad launch (dispatch_solve)
  mutable bool quad_id_lean = false;       // the last quad launch ran the structured identity-leaf loop (launch_quad)
  mutable std::string last_kernel_text;    // last_kernel with that loop and the build tag named
  mutable std::string quad_build;          // template arguments of the last quad launch (quad_build_tag below)
  mutable const char* last_kernel = "none";  // mapping the last control step / rollout was launched with (rmp2_last_kernel)
  std::string error;
};

// A step launch: plain, or -- when a completion fence is attached to the handle (rmp2_set_step_fence) -- with the
// fence as the dispatch's own completion signal (hipExtLaunchKernelGGL stop event): no separate packet behind the kernel.
#define RMP2_STEP_LAUNCH(h_, kern_, grid_, block_, bytes_, stream_, ...)                                            \
  do {                                                                                                              \
    if ((h_)->step_fence)                                                                                           \
      hipExtLaunchKernelGGL(kern_, grid_, block_, bytes_, stream_, nullptr, static_cast<hipEvent_t>((h_)->step_fence), 0, \
                            __VA_ARGS__);                                                                           \
    else                                                                                                            \
      hipLaunchKernelGGL(kern_, grid_, block_, bytes_, stream_, __VA_ARGS__);                                       \
  } while (0)

namespace rmp2 {
// f(std::integral_constant<int, S>) with S = n, the save slots of a program: the SLOTS argument of a kernel template.  rmp2_create
// refuses programs with more than 2.
template <class F>
auto with_slots(int n, F&& f) {
  switch (n) {
    case 0: return f(std::integral_constant<int, 0>());
    case 1: return f(std::integral_constant<int, 1>());
    default: return f(std::integral_constant<int, 2>());
  }
}

// rmp2_quad_tu.hip: one object per template size N and save/restore slot count of the program
#define RMP2_DECL_QUAD(NAME)                                                                                            \
  bool NAME(const rmp2_handle* h, const float* q, const float* qd, const float* goal, int gs, const ObsArgs& o,         \
            const OutArgs& out, const RolloutArgs& ro, int R, hipStream_t s)
RMP2_DECL_QUAD(launch_quad_n2_s0);
RMP2_DECL_QUAD(launch_quad_n2_s1);
RMP2_DECL_QUAD(launch_quad_n2_s2);
RMP2_DECL_QUAD(launch_quad_n9_s0);
RMP2_DECL_QUAD(launch_quad_n9_s1);
RMP2_DECL_QUAD(launch_quad_n9_s2);
#undef RMP2_DECL_QUAD
// rmp2_quad_pair_tu.hip: the control steps of two engines as ONE grid (a 2-dof and a 3..9-dof robot type on shared / ragged
// sphere tables: a mixed fleet shard); false = no fused instantiation for this pair, nothing was launched
bool launch_quad_pair(const rmp2_handle* ha, const float* qa, const float* qda, const float* goala, int gsa, const ObsArgs& oa,
                      const OutArgs& outa, int Ra, const rmp2_handle* hb, const float* qb, const float* qdb, const float* goalb,
                      int gsb, const ObsArgs& ob, const OutArgs& outb, int Rb, hipStream_t s);
// solve = PINV handles whose strict step is ONE quad launch: an inertia leaf (else every robot is rank deficient and would take
// the careful pass), <= 16 goal floats; symmetric sets are certified from the LDL^T of the elimination, the others from U and
// the largest multiplier (rmp2_quad.h)
// The instantiation of rmp2_step_quad_kernel a launch took, as text for rmp2_last_kernel: "[build n9 s1 w4 rollout ragged sym sph]" =
// N, SLOTS, MINW, ("staged": STAGE,) FLAVOR, OBS, SYM (sym | gen), CAP (sph | cap)(, "pt": PT).  Formed from the template arguments at
// the launch site, so that a test can tell which build it reached.
inline std::string quad_build_tag(int n, int slots, int minw, bool stage, bool cap, bool sym, int obs, int flavor, bool pt) {
  static const char* const kFlavor[] = {"general", "plain", "rollout"};
  static const char* const kObs[] = {"any", "none", "explicit", "shared", "ragged", "shared-link", "explicit-stream"};
  // (indexed by OBS + 1: rmp2_quad.h kObsAny = -1, the modes of include/rmp2.h, kObsSharedLink = 4, kObsExplicitStream = 5)
  static_assert(RMP2_OBS_NONE == 0 && RMP2_OBS_EXPLICIT_PAIRS == 1 && RMP2_OBS_SHARED_SPHERES == 2 && RMP2_OBS_RAGGED_SPHERES == 3 &&
                    kObsAny == -1 && kObsSharedLink == 4 && kObsExplicitStream == 5, "kObs");
  return "[build n" + std::to_string(n) + " s" + std::to_string(slots) + " w" + std::to_string(minw) + (stage ? " staged " : " ") +
         kFlavor[flavor] + " " + kObs[obs + 1] + (sym ? " sym" : " gen") + (cap ? " cap" : " sph") + (pt ? " pt]" : "]");
}
inline bool quad_certifies_strict(const rmp2_handle* h) {
  return h->strict && h->strict_certify && !h->likely_singular && h->n_template == 9 && h->goal_floats <= 16;
}
// ... and in the hex mapping (any template size: its Gauss-Jordan keeps the pivot rows for the same certificate)
inline bool hex_certifies_strict(const rmp2_handle* h) { return h->strict && h->strict_certify && !h->likely_singular; }
inline QuadHdr make_quad_hdr(const rmp2_handle* h) {
  return QuadHdr{h->n_ops_step, h->n_dof, h->n_id_leaves, h->n_leaves, h->goal_floats, h->n_leaf_ops, h->rev_mask,
                 h->hex_levels, h->n_fk_leaves, h->hex_is_chain, {h->dof_ops[0], h->dof_ops[1], h->dof_ops[2]}, h->cull_c0, h->strict ? 1 : 0,
                 h->prio_tail >= 0 ? h->prio_tail : 0, h->quad_skip_resolve ? 1 : 0, h->has_point ? 1 : 0, h->likely_singular ? 1 : 0,
                 h->stream_stagger, h->id_structured ? 1 : 0};
}
// rmp2_hex_tu.hip (false: the working set does not fit the CU's LDS -- the caller falls back to the quad mapping)
bool launch_hex_n2(const rmp2_handle* h, const float* q, const float* qd, const float* goal, int gs, const ObsArgs& o,
                   const OutArgs& out, const RolloutArgs& ro, int R, hipStream_t s);
bool launch_hex_n9(const rmp2_handle* h, const float* q, const float* qd, const float* goal, int gs, const ObsArgs& o,
                   const OutArgs& out, const RolloutArgs& ro, int R, hipStream_t s);
bool launch_hex_n16(const rmp2_handle* h, const float* q, const float* qd, const float* goal, int gs, const ObsArgs& o,
                    const OutArgs& out, const RolloutArgs& ro, int R, hipStream_t s);
// One call of the contact step, whichever entry point made it: everything any form's launch needs.  A form ignores the fields it
// has no use for (csr_offset / csr_index without LIST; planes / P in the sphere-only forms; ...).  Host only: the launchers spread
// it into their kernel's own parameter list, it never reaches a kernel.
struct ContactCall {
  float *q, *qd;
  const float* u;
  int accel;
  const float *lim, *qlo, *qhi;
  const float* spheres;
  int K;
  const int32_t *csr_offset, *csr_index;
  const float* planes;
  int P;
  const float* capsules;
  int C;
  const float* cylinders;
  int Y;
  const int32_t *cyl_offset, *cyl_index;
  int self_pairs;   // the cylinder forms: 0 -- the handle's self pairs are left out, none of their tables is passed to the kernel
  float d_act, dt;
  int substeps;
  float *qdd_out, *tau_out, *stop_out, *contact_out, *lambda_out;
  int32_t* pair_out;
  uint32_t* status_out;
  int R;
};
// rmp2_contacts_tu.hip: the contact step's kernels (rmp2_contacts.h), one object and one launcher per form and sphere source
// (table: the shared sphere table; lists: per-robot lists over a pool).
using ContactLauncher = void(const rmp2_handle* h, const ContactCall& c, hipStream_t s);
ContactLauncher launch_contacts_table, launch_contacts_lists;                  // spheres only
ContactLauncher launch_contacts_table_planes, launch_contacts_lists_planes;    // ... and half-spaces
ContactLauncher launch_contacts_table_capsules, launch_contacts_lists_capsules;   // ... and capsule obstacles
ContactLauncher launch_contacts_table_self, launch_contacts_lists_self;        // ... and the handle's self pairs
ContactLauncher launch_contacts_table_cylinders, launch_contacts_lists_cylinders;   // ... and the cylinder table
ContactLauncher launch_contacts_table_cylinder_lists, launch_contacts_lists_cylinder_lists;   // ... as per-robot cylinder lists
}  // namespace rmp2

// rmp2_contacts.h -- the plant's step with obstacle contacts (include/rmp2.h rmp2_dynamics_step_contacts).
//
// Frictionless, inelastic, velocity-level contacts between the robot's link capsules and a static shared table of spheres,
// solved together with the joint-limit stops of rmp2_joint_stops.h.  Per substep, at the state (q, qd): a, v* = qd + dt a and
// the velocity box (l, h) as there.  One kinematic walk over the program (id_visit, as fd_walk: the joints' world axes z_j and
// origins o_j are stored when the walk passes them) forms, for every frame f with a capsule and every sphere k,
//     X = the point of the capsule's world segment nearest the centre c_k,  n = (X - c_k) / |X - c_k|  (+z where X = c_k:
//     link_normal_length's convention),  gap g = |X - c_k| - r_k - r_f,
// keeps the pairs with g <= d_act -- at most kMaxContacts, the smallest gaps, ties to the lower pair index f K + k; the excess
// is counted -- and writes each kept pair's row at once:  J[j] = n . (z_j x (X - o_j))  (revolute ancestor dof j),  n . z_j
// (prismatic), 0 otherwise;  bound b = -max(g, 0) / dt.  The substep's velocity is
//     v = argmin 1/2 (v - v*)^T M (v - v*)   s.t.   l <= v <= h,   J_c v >= b_c,
// found by a primal active-set method over general rows a_i v >= beta_i (+e_j v >= l_j, -e_j v >= -h_j, J_c v >= b_c) from the
// feasible start v = 0 (b <= 0, l <= 0 <= h):
//   M is factored once per substep (in place, where fd_evaluate_saved stored it).  A row that enters the working set W gets its
//   column Y_i = M^-1 a_i.  Each iteration forms the Gram matrix G = A_W Y_W, factors it (Cholesky, row by row), solves
//   G mu = beta_W - A_W v*, x = v* + Y_W mu (dofs of W put on their bounds exactly);  if a row outside W is violated at x and
//   decreases along x - v: go to the first such row on the segment and add it (of rows met at the same point -- every pair
//   in penetration blocks at the start v = 0 -- the one that x violates most, relative to |a_i|_1);  else take x, drop from W
//   the most negative multiplier (never a dof with l_j == h_j), and stop when there is none.
//   A Gram pivot below kContactPivot x its diagonal entry (a row that is dependent on W to fp32 resolution), or a row that
//   would make W larger than the number of dofs: the row is left out and the substep ends at the current, feasible, iterate;
//   this and the iteration cap (kContactMaxIter; the iterate it leaves is feasible like every other) are reported as RMP2_STOP_CAPPED.  A row outside W counts as violated /
//   decreasing only beyond kContactTol x |a_i|_1 max|v*| (the box rows likewise, and x is clipped into the box when taken): two spheres on one spot give two identical rows, and the one outside
//   W must not block on the other's rounding.
// Every iterate is feasible (the box exactly, the contact rows to that tolerance).  A substep without a candidate runs
// rmp2_joint_stops.h's substep, expression for expression.
//
// Per-lane storage (pointer + stride: on the device LDS, lane-interleaved, word k of lane l at k * 64 + l; on the host a local
// array): U (the packed factor of M), the candidate rows J [8][N], the columns Y [N][N], the Gram factor and the multipliers.
// These are indexed at run time (LDS addresses are per lane); every index into a REGISTER array is a compile-time constant
// after unrolling -- dynamic picks are unrolled compares.  Host-compilable (tests/contacts_driver.cpp).
//
// Forms.  All are dynamics_step_contacts_robot<N, SLOTS, LIST, Pl, Cp, Sp, Cy>, one body with the differences under `if constexpr`:
// LIST says where the robot's SPHERES come from (SphereTable, the fleet's shared table, or SphereList, its own list over a shared
// pool) and is independent of everything else; Pl / Cp / Sp / Cy are a form object below or its empty No... twin.  The kernels at
// the end of this file (one per row of the table; rmp2_contacts_tu.hip instantiates each once per LIST, a code object each) build
// the form objects from their parameters and run dynamics_step_contacts_robot on the lane's robot (why each spells that out: the comment above the
// kernels).  A form's rows are numbered from its pair-index base (F frames, K / P / C / Y the pool or table sizes); the LDS words are per lane.
//
//   entry point rmp2_dynamics_step_  kernel rmp2_dynamics_step_              on                                  LDS words              pair-index base
//   contacts, contacts_lists         contacts_kernel<.., PLANES = false>     spheres                             contact_words(N)       0
//   contacts_planes                  contacts_kernel<.., PLANES = true>      + PlaneTable                        contact_words(N)       F K
//   contacts_capsules                contacts_capsules_kernel                + CapsuleTable                      contact_words(N)       F (K + 2 P)
//   contacts_self                    contacts_self_kernel                    + SelfPairs (the handle's)          contact_self_words(N)  F (K + 2 P + C)
//   contacts_cylinders               contacts_cylinders_kernel               + CylinderTable (SelfPairs by flag) contact_self_words(N)  F (K + 2 P + C) + F F
//   contacts_cylinder_lists          contacts_cylinder_lists_kernel          CylinderList in its place           contact_self_words(N)  F (K + 2 P + C) + F F
#pragma once
#include <type_traits>

#include "rmp2_joint_stops.h"

namespace rmp2 {

constexpr int kMaxContacts = RMP2_MAX_CONTACTS;
// Twice the worst iteration count of the fp64 restatement over every test fleet -- 17, on the stress catalogue of
// tests/contacts_scene.py (tests/test_contacts_host.py).
#ifndef RMP2_CONTACT_MAX_ITER
#define RMP2_CONTACT_MAX_ITER 34
#endif
constexpr int kContactMaxIter = RMP2_CONTACT_MAX_ITER;   // (the define: tests of the capped exit only)
constexpr float kContactPivot = 2.4e-7f;   // 4 x 2^-24: below it the pivot is its own rounding
constexpr float kContactTol = 1e-5f;

// words per lane: U, J, Y, the Gram factor, the multipliers
constexpr int contact_words(int n) { return fd_tri(n) + kMaxContacts * n + n * n + fd_tri(n) + n; }

template <int N>
__host__ __device__ inline float ct_get(const float (&a)[N], int j) {
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) r = i == j ? a[i] : r;
  return r;
}

// Where a robot's sphere records come from.  The candidate search and the step are written once over a source, which says how
// many records the robot has (count) and what the pair index f K + k counts in (pool); the arithmetic on a record is the same
// code for both, only the fetch differs (if constexpr on kList).
struct SphereRec {
  float c[3], r;
};

// The fleet's shared table: every record in table order, read at uniform addresses.
struct SphereTable {
  const float* spheres;
  int K;
  static constexpr bool kList = false;
  __host__ __device__ int count() const { return K; }
  __host__ __device__ int pool() const { return K; }
};

// One robot's list over a shared pool (rmp2_dynamics_step_contacts_lists): records pool[index[i]], i = 0 .. len - 1, in list
// order.  The addresses are the lane's own: a record is one 16-byte load (the pool is 16-byte aligned), and the cursor keeps the
// next entry's record and the index after it in flight while the arithmetic runs on the current one, so that neither of the two
// dependent fetches (index, then record) is waited for inside a trip.  scan() range-checks every entry BEFORE anything is read
// through it and empties an invalid list: the cursor never sees an entry that was not checked.
struct SphereList {
  const float* spheres;   // the pool [K][4]
  int K;
  const int32_t* index;   // the robot's entries
  int len;                // how many; < 0 or > RMP2_MAX_CONTACT_LIST: invalid
  static constexpr bool kList = true;
  __host__ __device__ int count() const { return len; }
  __host__ __device__ int pool() const { return K; }
  __host__ __device__ SphereRec record(int k) const {
    SphereRec r;
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 v = *reinterpret_cast<const float4*>(spheres + 4 * (size_t)k);
    r.c[0] = v.x, r.c[1] = v.y, r.c[2] = v.z, r.r = v.w;
#else
    __builtin_memcpy(&r, spheres + 4 * (size_t)k, sizeof(r));
#endif
    return r;
  }
  __host__ __device__ float scan(bool& invalid) {
    invalid = len < 0 || len > RMP2_MAX_CONTACT_LIST;
    if (invalid) len = 0;
    float p = 0.f;
    for (int i = 0; i < len; ++i) {
      const int k = index[i];
      if ((uint32_t)k >= (uint32_t)K) {   // (also a negative entry)
        invalid = true;
        continue;
      }
      const SphereRec r = record(k);
      p += r.c[0] * 0.f;
      p += r.c[1] * 0.f;
      p += r.c[2] * 0.f;
      p += r.r * 0.f;
    }
    if (invalid) len = 0;
    return p;
  }
  struct Cursor {
    SphereRec rec;    // the record of the entry that next() hands out next
    int k, k_next;    // that entry's index and the index after it
    __host__ __device__ void begin(const SphereList& l) {
      k = k_next = 0;
      rec = SphereRec{{0.f, 0.f, 0.f}, 0.f};
      if (l.len > 0) {
        k = l.index[0];
        rec = l.record(k);
      }
      if (l.len > 1) k_next = l.index[1];
    }
    // entry s's record and (returned) its index in the pool; the fetches of entry s + 1's record and of entry s + 2's index
    // are issued before the caller uses what it got
    __host__ __device__ int next(const SphereList& l, int s, float (&c)[3], float& rs) {
      c[0] = rec.c[0], c[1] = rec.c[1], c[2] = rec.c[2];
      rs = rec.r;
#if defined(__HIP_DEVICE_COMPILE__)
      // The four values enter the trip as the table's four loads do -- defined here, in this order -- and not as loop-carried
      // registers: the optimiser orders the operands of a sum by where its terms are defined, and the contraction into fma
      // follows that order, so as loop-carried values the dot products round differently from the table form's.  This leans on
      // the compiler; the guard is tests/test_gpu_contacts_lists.py
      // test_catalogue_in_one_launch_equals_the_shared_call_per_group_bit_for_bit, which fails when a compiler release orders
      // them otherwise.  The robust form -- explicit fmaf in id_dot, or contraction switched off -- changes the table kernel's
      // code and bits as well, and is left for a change that may do that.
      asm volatile("" : "+v"(c[0]));
      asm volatile("" : "+v"(c[1]));
      asm volatile("" : "+v"(c[2]));
      asm volatile("" : "+v"(rs));
#endif
      const int k_now = k;
      if (s + 1 < l.len) {
        k = k_next;
        rec = l.record(k);
      }
      if (s + 2 < l.len) k_next = l.index[s + 2];
      return k_now;
    }
  };
};

// Robot r's span of csr_index from csr_offset [R + 1]: the entries start at index + beg; returns their number, or -1 where the
// offsets give no list (a negative start or a negative length).  A length above RMP2_MAX_CONTACT_LIST is returned as it is:
// SphereList::scan refuses it.
__host__ __device__ inline int contact_list_span(const int32_t* csr_offset, int r, int& beg) {
  const int b = csr_offset[r], e = csr_offset[r + 1];
  beg = b < 0 ? 0 : b;
  return b < 0 || e < b ? -1 : e - b;
}

// Half-space obstacles beside the spheres (rmp2_dynamics_step_contacts_planes).  The routines below take the planes as a defaulted
// template parameter: with NoPlanes each `if constexpr (Pl::kOn)` is discarded and the code is what it is without planes.  PlaneTable: the fleet's records [P][4] = (n, d), free space n . x >= d, read at uniform
// addresses like the shared sphere table; F, the robot's frame count, places the plane rows' pair indices after the spheres':
// F K + 2 (f P + p) + e.
struct NoPlanes {
  static constexpr bool kOn = false;
};
struct PlaneTable {
  const float* planes;
  int P, F;
  static constexpr bool kOn = true;
};

// Capsule obstacles beside the spheres and the planes (rmp2_dynamics_step_contacts_capsules), a defaulted template parameter like
// the planes: with NoCapsules each `if constexpr (Cp::kOn)` is discarded.  CapsuleTable: the fleet's records [C][8] = (a, radius,
// b, 0), read like the shared sphere table; F and P, the robot's frame count and the call's plane count, place the capsule rows'
// pair indices after the spheres' and the planes': F K + 2 F P + f C + c.  A capsule pair is the sphere pair (Y, radius), Y the
// point of the obstacle's axis nearest the link's axis (segment_segment): the sphere trip runs on it, there is no other row code.
struct NoCapsules {
  static constexpr bool kOn = false;
};
struct CapsuleTable {
  const float* capsules;
  int C, F, P;
  static constexpr bool kOn = true;
};

// Self contacts between the robot's own link capsules (rmp2_dynamics_step_contacts_self), a defaulted template parameter like the
// capsules: with NoSelfPairs each `if constexpr (Sp::kOn)` is discarded.  SelfPairs: the handle's pair list as three int32 tables,
// constants of the program formed on the host (rmp2_set_contact_self_pairs) and read at uniform addresses.  Of a pair {i, j} the
// frame the walk visits later is the LINK f, the other the PARTNER e.  slot [n_ops]: the partner slot of op k's frame, or -1;
// begin [n_ops + 1]: op k's pairs (its frame in the link role) are the records begin[k] .. begin[k + 1] - 1;  rec [n][4] =
// (the partner's slot, the partner's frame e, anc(f) & ~anc(e), anc(e) & ~anc(f)).  When the walk passes a partner frame it stores
// the world segment's two ends in the slot (6 words per lane at seg, word w of the lane at seg[w * stride]); at a link frame each
// pair is one more trip after the spheres and the obstacle capsules: the capsule trip with the stored segment (A_e, A_e + D_e, r_e)
// where the obstacle (C_0, C_1, r_c) stood.  The row's entries are the one-body row's under the first mask and, across a branch,
// -n . (z_j x (Y - o_j)) (revolute; -n . z_j prismatic) under the second; dofs common to both links are exactly 0.  Pair index:
// F (K + 2 P + C) + f F + e.  n == 0: no pairs, nothing is read.
struct NoSelfPairs {
  static constexpr bool kOn = false;
};
struct SelfPairs {
  const int32_t* slot;
  const int32_t* begin;
  const int32_t* rec;
  int n, F;
  float* seg;   // (set by dynamics_step_contacts_robot: the solver's columns, free during the search)
  static constexpr bool kOn = true;
};
constexpr int kMaxSelfFrames = RMP2_MAX_CONTACT_SELF_FRAMES;
// words per lane of the self forms: the partner segments lie over Y, the Gram factor and the multipliers, which only the solver
// writes, after the search of the same substep.  N = 9: 6 * 22 = 132 of those 135 words, no word more than contact_words(9);
// N = 2: that region has 9 words, the segments reach past it.
constexpr int contact_self_words(int n) {
  const int need = fd_tri(n) + kMaxContacts * n + 6 * kMaxSelfFrames;
  return need > contact_words(n) ? need : contact_words(n);
}

// Flat-capped cylinder obstacles beside all of the above (rmp2_dynamics_step_contacts_cylinders), a defaulted template parameter
// like the self pairs: with NoCylinders each `if constexpr (Cy::kOn)` is discarded.  CylinderTable: the fleet's records [Y][8] =
// (centre, radius, unit axis, half height) -- the RMP2_PRIM_CYLINDER record the policy reads --, read like the shared sphere table;
// F, P and C place the cylinder rows' pair indices after the self block: F (K + 2 P + C) + F F + f Y + y.  A cylinder pair is NOT a
// sphere pair at the nearest point: segment_cylinder (rmp2_device.h) gives the point X of the link's axis, the outward normal n of
// the cylinder's surface at its nearest point and the signed distance sd, and the trip hands (X, n, g = sd - r_f) to the one
// keep-and-write statement as they are -- the surface's normal does not flip in penetration and is defined at g = 0.
// The cull in front of the bisection: the solid lies inside the ball (centre, rho = sqrt(r^2 + h^2)), so with X_c the point of the
// link's segment nearest the centre every point of the segment has g >= L = |X_c - centre| - rho - r_f; a trip with
// L > d_act + 1e-4 (1 + |X_c - centre| + rho) (a hundred times the rounding of L) cannot qualify and is skipped; a NaN L does not
// skip.  -DRMP2_CYLINDER_NO_CULL (tests/contacts_driver.cpp and tools/contact_cylinders_timing.py only) leaves it out.
struct NoCylinders {
  static constexpr bool kOn = false;
  static constexpr bool kList = false;
};
struct CylinderTable {
  const float* cylinders;
  int Y, F, P, C;
  static constexpr bool kOn = true;
  static constexpr bool kList = false;
};

// One robot's list over a shared pool of cylinder records (rmp2_dynamics_step_contacts_cylinder_lists): records pool[index[i]],
// i = 0 .. len - 1, in list order, as SphereList is for the spheres.  The arithmetic of a cylinder trip is CylinderTable's; the
// fetch is a gather -- a record is two 16-byte loads at the lane's own address (the pool is 16-byte aligned) -- and the trip count
// is the lane's own.  The cursor (begin / next) keeps the next entry's record and the index after it in flight while the current
// entry is evaluated.  scan() range-checks every entry BEFORE anything is read through it, adds the robot's own records to the poison sum
// and empties an invalid list: the cursor never sees an entry that was not checked.  Y is the POOL's size and the pair index counts
// in it: F (K + 2 P + C) + F F + f Y + (the pool index).
struct CylinderRec {
  float4 a, b;   // (centre, radius), (unit axis, half height)
};
struct CylinderList {
  const float* cylinders;   // the pool [Y][8]
  int Y;
  const int32_t* index;     // the robot's entries
  int len;                  // how many; < 0 or > RMP2_MAX_CYLINDER_LIST: invalid
  int F, P, C;
  // the cursor (begin / next): the record of the entry that next() hands out next, that entry's index and the index after it, and
  // the index of the entry handed out last.  State of the list itself -- the routines that walk it take the list by value
  CylinderRec rec;
  int k, k_next, k_now;
  float held[8];
  static constexpr bool kOn = true;
  static constexpr bool kList = true;
  __host__ __device__ CylinderRec record(int k) const {
    CylinderRec r;
#if defined(__HIP_DEVICE_COMPILE__)
    const float4* p = reinterpret_cast<const float4*>(cylinders + 8 * (size_t)k);
    r.a = p[0];
    r.b = p[1];
#else
    __builtin_memcpy(&r, cylinders + 8 * (size_t)k, sizeof(r));
#endif
    return r;
  }
  __host__ __device__ float scan(bool& invalid) {
    invalid = len < 0 || len > RMP2_MAX_CYLINDER_LIST;
    if (invalid) len = 0;
    float p = 0.f;
    for (int i = 0; i < len; ++i) {
      const int k = index[i];
      if ((uint32_t)k >= (uint32_t)Y) {   // (also a negative entry, and every entry when Y == 0)
        invalid = true;
        continue;
      }
      const CylinderRec r = record(k);
      p += r.a.x * 0.f;
      p += r.a.y * 0.f;
      p += r.a.z * 0.f;
      p += r.a.w * 0.f;
      p += r.b.x * 0.f;
      p += r.b.y * 0.f;
      p += r.b.z * 0.f;
      p += r.b.w * 0.f;
    }
    if (invalid) len = 0;
    return p;
  }
  __host__ __device__ void begin() {
    k = k_next = k_now = 0;
    rec.a = rec.b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (len > 0) {
      k = index[0];
      rec = record(k);
    }
    if (len > 1) k_next = index[1];
  }
  // entry j's record -- its eight words in `held`, returned, where the table form has a pointer into the table -- and its index in
  // the pool in k_now; the fetches of entry j + 1's record and of entry j + 2's index are issued before the caller uses what it got
  __host__ __device__ const float* next(int j) {
    held[0] = rec.a.x, held[1] = rec.a.y, held[2] = rec.a.z, held[3] = rec.a.w;
    held[4] = rec.b.x, held[5] = rec.b.y, held[6] = rec.b.z, held[7] = rec.b.w;
#if defined(__HIP_DEVICE_COMPILE__)
    // as SphereList::Cursor::next: the eight words enter the trip defined here, in the table form's load order, and not as
    // loop-carried registers, so that the contraction into fma meets them where the table form's loads stand
    asm volatile("" : "+v"(held[0]));
    asm volatile("" : "+v"(held[1]));
    asm volatile("" : "+v"(held[2]));
    asm volatile("" : "+v"(held[3]));
    asm volatile("" : "+v"(held[4]));
    asm volatile("" : "+v"(held[5]));
    asm volatile("" : "+v"(held[6]));
    asm volatile("" : "+v"(held[7]));
#endif
    k_now = k;
    if (j + 1 < len) {
      k = k_next;
      rec = record(k);
    }
    if (j + 2 < len) k_next = index[j + 2];
    return held;
  }
};

// The slot of a qualifying candidate (gap g, pair index idx) among the kept ones: a free slot, or the kept candidate of largest
// (gap, index) when the new one is smaller, or -1.  The rule of the sphere trip below, which keeps its own inline statement of it
// (its code is not to change); the plane trip calls this.
__host__ __device__ inline int contact_slot(float g, int idx, int& count, float (&cgap)[kMaxContacts], int (&cidx)[kMaxContacts]) {
  int put = -1;
  if (count < kMaxContacts) {
    put = count++;
  } else {
    float wg = cgap[0];
    int wi = cidx[0], ws = 0;
#pragma unroll
    for (int e = 1; e < kMaxContacts; ++e)
      if (cgap[e] > wg || (cgap[e] == wg && cidx[e] > wi)) {
        wg = cgap[e];
        wi = cidx[e];
        ws = e;
      }
    if (g < wg || (g == wg && idx < wi)) put = ws;
  }
  if (put < 0) return put;
#pragma unroll
  for (int e = 0; e < kMaxContacts; ++e)
    if (e == put) {
      cgap[e] = g;
      cidx[e] = idx;
    }
  return put;
}

// The candidate search and the rows of one robot at q.  caps: [n_frames][8] (a, radius, b, 0) in frame coordinates, read at
// uniform addresses; src: the robot's spheres (above).  Jr: the rows' storage.  cgap / cidx: gap and pair index per slot (cidx
// -1: empty).  Returns the number of candidates kept; excess: how many more qualified.
template <int N, int SLOTS, class Src, class Pl = NoPlanes, class Cp = NoCapsules, class Sp = NoSelfPairs, class Cy = NoCylinders>
__host__ __device__ inline int contact_candidates_from(const DevOp* ops, int n_ops, const float* caps, Src src,
                                                       float d_act, const float (&q)[N], float* Jr, int stride,
                                                       float (&cgap)[kMaxContacts], int (&cidx)[kMaxContacts], int& excess,
                                                       Pl pl = Pl{}, Cp oc = Cp{}, Sp sp = Sp{}, Cy cy = Cy{}) {
  static_assert(!Sp::kOn || (Pl::kOn && Cp::kOn), "the self forms run with the planes and the capsules on");
  static_assert(!Cy::kOn || (Pl::kOn && Cp::kOn && Sp::kOn), "the cylinder forms run with the planes, the capsules and the self pairs on");
  const int K = src.count();   // the robot's records (the pair index is made of src.pool())
  float ax[N][3], org[N][3];
#pragma unroll
  for (int j = 0; j < N; ++j)
    for (int k = 0; k < 3; ++k) ax[j][k] = org[j][k] = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxContacts; ++c) {
    cgap[c] = 0.f;
    cidx[c] = -1;
  }
  int count = 0, total = 0;
  uint32_t revolute = 0u;
  const float still[3] = {0.f, 0.f, 0.f};
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
    id_visit(cur, op, ct_get<N>(q, qi), 0.f, 0.f, op.restore == -2, still, z);
    if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.save == s) slot[s] = cur;
    }
    if (qi >= 0) {
      if (op.jtype == RMP2_JOINT_REVOLUTE) revolute |= 1u << qi;
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (j == qi)
          for (int c = 0; c < 3; ++c) {
            ax[j][c] = z[c];
            org[j][c] = cur.p[c];
          }
    }
    const float* cp = caps + (size_t)op.frame * 8;
    bool has = false;
    for (int i = 0; i < 8; ++i) has = has || cp[i] != 0.f;
    if constexpr (Pl::kOn || Cp::kOn) {   // (a frame without spheres still meets the planes and the capsules)
      if (!has) continue;
    } else {
      if (!has || K <= 0) continue;
    }
    const float al[3] = {cp[0], cp[1], cp[2]}, dl[3] = {cp[4] - cp[0], cp[5] - cp[1], cp[6] - cp[2]};
    const float rf = cp[3];
    float A[3], D[3];
    for (int i = 0; i < 3; ++i) {
      A[i] = cur.R[3 * i + 0] * al[0] + cur.R[3 * i + 1] * al[1] + cur.R[3 * i + 2] * al[2] + cur.p[i];
      D[i] = cur.R[3 * i + 0] * dl[0] + cur.R[3 * i + 1] * dl[1] + cur.R[3 * i + 2] * dl[2];
    }
    const float dd = id_dot(D, D);
    const float inv_dd = dd > 0.f ? 1.f / dd : 0.f;
    const uint32_t mask = op.anc_mask;
    int self_begin = 0, self_trips = 0;   // the pairs with this frame in the link role
    if constexpr (Sp::kOn) {
      if (sp.n > 0) {
        const int sl = sp.slot[k];
        if (sl >= 0)   // a partner of frames to come: its world segment's ends, per lane
          for (int i = 0; i < 3; ++i) {
            sp.seg[(size_t)(6 * sl + i) * stride] = A[i];
            sp.seg[(size_t)(6 * sl + 3 + i) * stride] = A[i] + D[i];
          }
        self_begin = sp.begin[k];
        self_trips = sp.begin[k + 1] - self_begin;
      }
    }
    if constexpr (Pl::kOn) {
      // the planes: one row per end of the segment (a zero-length capsule: the end 0 only), the normal the plane's as given
      const int ends = (D[0] == 0.f && D[1] == 0.f && D[2] == 0.f) ? 1 : 2;
      for (int p = 0; p < pl.P; ++p) {
        const float nu[3] = {pl.planes[4 * p + 0], pl.planes[4 * p + 1], pl.planes[4 * p + 2]};
        const float pd = pl.planes[4 * p + 3];
        for (int e = 0; e < ends; ++e) {
          float X[3];
          for (int i = 0; i < 3; ++i) X[i] = e ? A[i] + D[i] : A[i];
          const float g = id_dot(nu, X) - pd - rf;
          if (!(g <= d_act)) continue;   // (also a NaN gap)
          ++total;
          const int idx = pl.F * src.pool() + 2 * (op.frame * pl.P + p) + e;
          const int put = contact_slot(g, idx, count, cgap, cidx);
          if (put < 0) continue;
          float* row = Jr + (size_t)put * N * stride;
#pragma unroll
          for (int j = 0; j < N; ++j) {
            float val = 0.f;
            if ((mask >> j) & 1u) {
              if ((revolute >> j) & 1u) {
                const float d[3] = {X[0] - org[j][0], X[1] - org[j][1], X[2] - org[j][2]};
                float zx[3];
                id_cross(ax[j], d, zx);
                val = id_dot(nu, zx);
              } else {
                val = id_dot(nu, ax[j]);
              }
            }
            row[j * stride] = val;
          }
        }
      }
    }
    SphereList::Cursor cursor;
    if constexpr (Src::kList) cursor.begin(src);
    int trips = K;   // with capsules: the robot's K spheres, then the C capsules, through the one trip body
    if constexpr (Cp::kOn) trips += oc.C;
    if constexpr (Sp::kOn) trips += self_trips;   // ... then its self pairs
    const int cyl_first = trips;                  // ... then the Y cylinders
    if constexpr (Cy::kList) {   // (the robot's own cylinders: the lane's trip count)
      cy.begin();
      trips += cy.len;
    } else if constexpr (Cy::kOn) {
      trips += cy.Y;
    }
    for (int s = 0; s < trips; ++s) {
      float c[3], rs;
      int sk = s;   // the record's index in the pool
      bool cylinder = false;
      if constexpr (Cy::kOn) cylinder = s >= cyl_first;
      bool capsule = false;
      if constexpr (Cp::kOn) capsule = s >= K && !cylinder;
      bool self = false;
      int se = 0;               // the partner's frame
      uint32_t mf = 0u, me = 0u;   // the dofs that move the link alone, the partner alone
      if constexpr (Sp::kOn) {
        self = s >= K + oc.C && !cylinder;
        capsule = capsule && !self;
      }
      if (cylinder) {   // (the record is read where the trip forms X, n and g, below)
      } else if (self) {
        if constexpr (Sp::kOn) {   // the capsule trip on the partner's stored segment
          const int32_t* pr = sp.rec + 4 * (size_t)(self_begin + (s - K - oc.C));
          se = pr[1];
          mf = (uint32_t)pr[2], me = (uint32_t)pr[3];
          const float* ce = caps + (size_t)se * 8;
          bool ehas = false;
          for (int i = 0; i < 8; ++i) ehas = ehas || ce[i] != 0.f;
          if (!ehas) continue;   // (a partner without a capsule: its slot was never written)
          const float* sg = sp.seg + (size_t)(6 * pr[0]) * stride;
          const float C0[3] = {sg[0], sg[stride], sg[2 * stride]}, C1[3] = {sg[3 * stride], sg[4 * stride], sg[5 * stride]};
          const float B[3] = {A[0] + D[0], A[1] + D[1], A[2] + D[2]};
          float sl, to;
          segment_segment(A, B, C0, C1, sl, to);
          for (int i = 0; i < 3; ++i) c[i] = C0[i] + to * (C1[i] - C0[i]);
          rs = ce[3];
        }
      } else if (capsule) {
        if constexpr (Cp::kOn) {   // the sphere (Y, radius): Y the point of the obstacle's axis nearest the link's axis
          const float* rec = oc.capsules + 8 * (size_t)(s - K);
          const float C0[3] = {rec[0], rec[1], rec[2]}, C1[3] = {rec[4], rec[5], rec[6]};
          const float B[3] = {A[0] + D[0], A[1] + D[1], A[2] + D[2]};
          float sl, to;
          segment_segment(A, B, C0, C1, sl, to);
          for (int i = 0; i < 3; ++i) c[i] = C0[i] + to * (C1[i] - C0[i]);
          rs = rec[3];
        }
      } else if constexpr (Src::kList) {
        sk = cursor.next(src, s, c, rs);
      } else {
        c[0] = src.spheres[4 * s + 0], c[1] = src.spheres[4 * s + 1], c[2] = src.spheres[4 * s + 2];
        rs = src.spheres[4 * s + 3];
      }
      float X[3], n[3], len, g;   // the point on the link's axis, the normal (of length len) and the gap
      if (cylinder) {
        if constexpr (Cy::kOn) {   // X, the surface's unit normal and the signed distance, from segment_cylinder as they are
          const float* rec;   // the record's eight words: in the table, or -- a list -- fetched through the cursor
          if constexpr (Cy::kList) rec = cy.next(s - cyl_first);
          else rec = cy.cylinders + 8 * (size_t)(s - cyl_first);
          const float4 ra = make_float4(rec[0], rec[1], rec[2], rec[3]), rb = make_float4(rec[4], rec[5], rec[6], rec[7]);
#ifndef RMP2_CYLINDER_NO_CULL
          {   // the solid lies in the ball (centre, rho): no point of the segment is nearer than L (see CylinderTable)
            const float relc[3] = {ra.x - A[0], ra.y - A[1], ra.z - A[2]};
            float tc = id_dot(relc, D) * inv_dd;
            tc = fminf(fmaxf(tc, 0.f), 1.f);
            const float dv[3] = {A[0] + tc * D[0] - ra.x, A[1] + tc * D[1] - ra.y, A[2] + tc * D[2] - ra.z};
            const float dist = sqrtf(id_dot(dv, dv));
            const float rho = sqrtf(ra.w * ra.w + rb.w * rb.w);
            const float L = dist - rho - rf;
            if (L > d_act + 1e-4f * (1.f + dist + rho)) continue;   // (a NaN L goes on)
          }
#endif
          float Yp[3], sd;
          segment_cylinder(ra, rb, A, D, X, Yp, n, sd);
          len = 1.f;
          g = sd - rf;
        }
      } else {
        const float rel[3] = {c[0] - A[0], c[1] - A[1], c[2] - A[2]};
        float t = id_dot(rel, D) * inv_dd;
        t = fminf(fmaxf(t, 0.f), 1.f);
        for (int i = 0; i < 3; ++i) {
          X[i] = A[i] + t * D[i];
          n[i] = X[i] - c[i];
        }
        const float dn = sqrtf(id_dot(n, n));
        len = link_normal_length(n);   // (+z and 1 where the centre lies on the axis)
        g = dn - rs - rf;
      }
      if (!(g <= d_act)) continue;   // (also a NaN gap)
      ++total;
      int idx = op.frame * src.pool() + sk;
      if constexpr (Cp::kOn) idx = capsule ? oc.F * (src.pool() + 2 * oc.P) + op.frame * oc.C + (s - K) : idx;
      if constexpr (Sp::kOn) idx = self ? oc.F * (src.pool() + 2 * oc.P + oc.C) + op.frame * sp.F + se : idx;
      if constexpr (Cy::kList)   // (the record's index in the POOL, of Y records)
        idx = cylinder ? cy.F * (src.pool() + 2 * cy.P + cy.C) + cy.F * cy.F + op.frame * cy.Y + cy.k_now : idx;
      else if constexpr (Cy::kOn)   // after the self block, which is reserved whether or not self pairs are on
        idx = cylinder ? cy.F * (src.pool() + 2 * cy.P + cy.C) + cy.F * cy.F + op.frame * cy.Y + (s - cyl_first) : idx;
      int put = -1;
      if (count < kMaxContacts) {
        put = count++;
      } else {   // the kept pair of largest (gap, index); it goes if the new pair is smaller
        float wg = cgap[0];
        int wi = cidx[0], ws = 0;
#pragma unroll
        for (int e = 1; e < kMaxContacts; ++e)
          if (cgap[e] > wg || (cgap[e] == wg && cidx[e] > wi)) {
            wg = cgap[e];
            wi = cidx[e];
            ws = e;
          }
        if (g < wg || (g == wg && idx < wi)) put = ws;
      }
      if (put < 0) continue;
#pragma unroll
      for (int e = 0; e < kMaxContacts; ++e)
        if (e == put) {
          cgap[e] = g;
          cidx[e] = idx;
        }
      const float inv = 1.f / len;
      const float nu[3] = {n[0] * inv, n[1] * inv, n[2] * inv};
      float* row = Jr + (size_t)put * N * stride;
      uint32_t lmask = mask;   // a self pair: the dofs that move the link and not the partner
      if constexpr (Sp::kOn) lmask = self ? mf : mask;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        float val = 0.f;
        if ((lmask >> j) & 1u) {
          if ((revolute >> j) & 1u) {
            const float d[3] = {X[0] - org[j][0], X[1] - org[j][1], X[2] - org[j][2]};
            float zx[3];
            id_cross(ax[j], d, zx);
            val = id_dot(nu, zx);
          } else {
            val = id_dot(nu, ax[j]);
          }
        }
        if constexpr (Sp::kOn) {   // the second body, across a branch: the dofs that move the partner and not the link
          if (self && ((me >> j) & 1u)) {
            if ((revolute >> j) & 1u) {
              const float d[3] = {c[0] - org[j][0], c[1] - org[j][1], c[2] - org[j][2]};
              float zx[3];
              id_cross(ax[j], d, zx);
              val = -id_dot(nu, zx);
            } else {
              val = -id_dot(nu, ax[j]);
            }
          }
        }
        row[j * stride] = val;
      }
    }
  }
  excess = total - count;
  return count;
}

// (the shared table: [K][4] read at uniform addresses)
template <int N, int SLOTS>
__host__ __device__ inline int contact_candidates(const DevOp* ops, int n_ops, const float* caps, const float* spheres, int K,
                                                  float d_act, const float (&q)[N], float* Jr, int stride,
                                                  float (&cgap)[kMaxContacts], int (&cidx)[kMaxContacts], int& excess) {
  return contact_candidates_from<N, SLOTS>(ops, n_ops, caps, SphereTable{spheres, K}, d_act, q, Jr, stride, cgap, cidx, excess);
}

// Row ids: [0, N) +e_j v >= l_j;  [N, 2N) -e_j v >= -h_j;  2N + c: J_c v >= b_c.
template <int N>
__host__ __device__ inline float ct_row_dot(int r, const float* Jr, int stride, const float (&x)[N]) {
  if (r < N) return ct_get<N>(x, r);
  if (r < 2 * N) return -ct_get<N>(x, r - N);
  const float* row = Jr + (size_t)(r - 2 * N) * N * stride;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) s += row[j * stride] * x[j];
  return s;
}

template <int N>
__host__ __device__ inline float ct_row_dot_col(int r, const float* Jr, const float* Yk, int stride) {
  if (r < N) return Yk[r * stride];
  if (r < 2 * N) return -Yk[(r - N) * stride];
  const float* row = Jr + (size_t)(r - 2 * N) * N * stride;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) s += row[j * stride] * Yk[j * stride];
  return s;
}

__host__ __device__ inline int ct_slot(uint64_t wl, int i) { return (int)((wl >> (6 * i)) & 63u); }

// The velocity of one substep with candidates.  U: the factor of M (fd_cholesky's).  nc candidates with bounds cb.  v: out, the
// minimiser (or the feasible iterate at which the solver stopped).  sigma: the stops' multipliers (M (v - v*) = sigma + J^T
// lamc), lamc: the contacts'.  Returns the number of iterations; capped: stopped before optimality (see the head).
template <int N>
__host__ __device__ inline int contacts_solve(const float* U, const float* Jr, float* Yw, float* Lw, float* mu, int stride,
                                              const float (&vstar)[N], const float (&lb)[N], const float (&ub)[N], int nc,
                                              const float (&cb)[kMaxContacts], float (&v)[N], float (&sigma)[N],
                                              float (&lamc)[kMaxContacts], bool& capped) {
  static_assert(6 * N <= 64 && 2 * N + kMaxContacts <= 64, "the working set is packed into 64 bits, 6 per slot");
  int m = 0, it = 0;
  uint64_t wl = 0u;      // the rows of W, slot by slot
  uint64_t inW = 0u;     // bit r: row r is in W
  capped = false;
  float vmax = 0.f;   // the velocity scale of the problem
#pragma unroll
  for (int j = 0; j < N; ++j) {
    v[j] = 0.f;
    vmax = fmaxf(vmax, fabsf(vstar[j]));
  }
  for (;;) {
    if (it >= kContactMaxIter) {
      capped = true;
      break;
    }
    ++it;
    // G = A_W Y_W = L L^T, row by row; the diagonal holds 1 / L_ii
    bool refuse = false;
    for (int i = 0; i < m; ++i) {
      const int ri = ct_slot(wl, i);
      float* Li = Lw + (size_t)(i * (i + 1) / 2) * stride;
      for (int k = 0; k <= i; ++k) {
        const float g = ct_row_dot_col<N>(ri, Jr, Yw + (size_t)k * N * stride, stride);
        const float* Lk = Lw + (size_t)(k * (k + 1) / 2) * stride;
        float s = g;
        for (int p = 0; p < k; ++p) s -= Li[p * stride] * Lk[p * stride];
        if (k < i) {
          Li[k * stride] = s * Lk[k * stride];
        } else {
          if (!(s > kContactPivot * g) || !(s <= FLT_MAX)) refuse = true;
          Li[i * stride] = 1.f / sqrtf(s);
        }
      }
    }
    if (refuse) {   // the row added last depends on the others: it stays out, the step ends here
      --m;
      inW &= ~(1ull << ct_slot(wl, m));
      capped = true;
      break;
    }
    // G mu = beta_W - A_W v*
    for (int i = 0; i < m; ++i) {
      const int ri = ct_slot(wl, i);
      const float beta = ri < N ? ct_get<N>(lb, ri) : (ri < 2 * N ? -ct_get<N>(ub, ri - N) : ct_get<kMaxContacts>(cb, ri - 2 * N));
      float s = beta - ct_row_dot<N>(ri, Jr, stride, vstar);
      const float* Li = Lw + (size_t)(i * (i + 1) / 2) * stride;
      for (int p = 0; p < i; ++p) s -= Li[p * stride] * mu[p * stride];
      mu[i * stride] = s * Li[i * stride];
    }
    for (int i = m - 1; i >= 0; --i) {
      float s = mu[i * stride];
      for (int p = i + 1; p < m; ++p) s -= Lw[(size_t)(p * (p + 1) / 2 + i) * stride] * mu[p * stride];
      mu[i * stride] = s * Lw[(size_t)(i * (i + 1) / 2 + i) * stride];
    }
    float x[N];
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = vstar[j];
    for (int i = 0; i < m; ++i) {
      const float mi = mu[i * stride];
      const float* Yi = Yw + (size_t)i * N * stride;
#pragma unroll
      for (int j = 0; j < N; ++j) x[j] += mi * Yi[j * stride];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {   // (a dof of W stays on its bound exactly)
      if ((inW >> j) & 1u) x[j] = lb[j];
      if ((inW >> (N + j)) & 1u) x[j] = ub[j];
      // W spans the dofs: every row of W is active at v, so the equality problem's solution IS v; what x differs by is the
      // rounding of an often ill-conditioned Gram solve (two contacts on neighbouring links), and must not move the iterate
      if (m == N) x[j] = v[j];
    }
    // the first row outside W that the segment from v to x meets
    // (ties -- rows that block at once, as every pair in penetration does from the start v = 0 -- go to the row that x
    // violates most, relative to |a_i|_1: the rows of a cluster of spheres on one link are nearly parallel, and the deepest of
    // them in W satisfies most of the others, where adding them in index order fills W with near-dependent rows)
    float alpha = 2.f, bval = 0.f, viol = 0.f;
    int brow = -1;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool in = ((inW >> j) | (inW >> (N + j))) & 1u;
      const bool below = x[j] < lb[j] - kContactTol * vmax, above = x[j] > ub[j] + kContactTol * vmax;
      if (!in && (below || above)) {
        const float b = below ? lb[j] : ub[j];
        float a = (b - v[j]) / (x[j] - v[j]);
        a = a < 0.f ? 0.f : a;
        const float w = fabsf(x[j] - b);
        if (a < alpha || (a == alpha && w > viol)) {
          alpha = a;
          viol = w;
          bval = b;
          brow = below ? j : N + j;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kMaxContacts; ++c)
      if (c < nc && !((inW >> (2 * N + c)) & 1u)) {
        const float* row = Jr + (size_t)c * N * stride;
        float jx = 0.f, jv = 0.f, jp = 0.f, rn = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const float r = row[j * stride];
          jx += r * x[j];
          jv += r * v[j];
          jp += r * (x[j] - v[j]);
          rn += fabsf(r);
        }
        const float scale = rn * vmax;
        if (jx < cb[c] - kContactTol * (scale + fabsf(cb[c])) && jp < -kContactTol * scale) {
          float a = (jv - cb[c]) / -jp;
          a = a < 0.f ? 0.f : a;
          const float w = (cb[c] - jx) / rn;
          if (a < alpha || (a == alpha && w > viol)) {
            alpha = a;
            viol = w;
            brow = 2 * N + c;
          }
        }
      }
    if (brow >= 0) {
      alpha = alpha < 0.f ? 0.f : (alpha > 1.f ? 1.f : alpha);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const bool in = ((inW >> j) | (inW >> (N + j))) & 1u;
        float t = v[j] + alpha * (x[j] - v[j]);
        t = t < lb[j] ? lb[j] : (t > ub[j] ? ub[j] : t);   // (a rounding must not leave the box)
        v[j] = (brow == j || brow == N + j) ? bval : (in ? v[j] : t);
      }
      if (m >= N) {   // (W already spans the dofs: only a rounding can ask for more)
        capped = true;
        break;
      }
      float y[N];
      const float* row = Jr + (size_t)(brow >= 2 * N ? brow - 2 * N : 0) * N * stride;
#pragma unroll
      for (int j = 0; j < N; ++j) y[j] = brow == j ? 1.f : (brow == N + j ? -1.f : (brow >= 2 * N ? row[j * stride] : 0.f));
      {
        float Ul[fd_tri(N)];
#pragma unroll
        for (int k = 0; k < fd_tri(N); ++k) Ul[k] = U[k * stride];
        fd_solve<N>(Ul, y);
      }
      float* Ym = Yw + (size_t)m * N * stride;
#pragma unroll
      for (int j = 0; j < N; ++j) Ym[j * stride] = y[j];
      mu[m * stride] = 0.f;
      wl = (wl & ~(63ull << (6 * m))) | ((uint64_t)brow << (6 * m));
      inW |= 1ull << brow;
      ++m;
      continue;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = x[j] < lb[j] ? lb[j] : (x[j] > ub[j] ? ub[j] : x[j]);   // (a rounding, below the tolerance)
    float worst = 0.f;
    int drop = -1;
    for (int i = 0; i < m; ++i) {
      const int ri = ct_slot(wl, i);
      const int j = ri < N ? ri : ri - N;
      const bool locked = ri < 2 * N && ct_get<N>(lb, j) == ct_get<N>(ub, j);
      const float mi = mu[i * stride];
      if (!locked && mi < worst) {
        worst = mi;
        drop = i;
      }
    }
    if (drop < 0) break;
    inW &= ~(1ull << ct_slot(wl, drop));
    for (int i = drop; i + 1 < m; ++i) {
      const float* Yn = Yw + (size_t)(i + 1) * N * stride;
      float* Yi = Yw + (size_t)i * N * stride;
#pragma unroll
      for (int j = 0; j < N; ++j) Yi[j * stride] = Yn[j * stride];
      mu[i * stride] = mu[(i + 1) * stride];
      const uint64_t r = (uint64_t)ct_slot(wl, i + 1);
      wl = (wl & ~(63ull << (6 * i))) | (r << (6 * i));
    }
    --m;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) sigma[j] = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxContacts; ++c) lamc[c] = 0.f;
  for (int i = 0; i < m; ++i) {
    const int ri = ct_slot(wl, i);
    const float mi = mu[i * stride];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if (ri == j) sigma[j] += mi;
      if (ri == N + j) sigma[j] -= mi;
    }
#pragma unroll
    for (int c = 0; c < kMaxContacts; ++c)
      if (ri == 2 * N + c) lamc[c] = fmaxf(mi, 0.f);   // (negative only where the solver stopped early)
  }
  return it;
}

template <bool LIST>
__host__ __device__ inline auto contact_source(const float* spheres, int K, const int32_t* list, int list_len) {
  if constexpr (LIST) return SphereList{spheres, K, list, list_len};
  else return SphereTable{spheres, K};
}

// rmp2_dynamics_step_contacts of one robot, and with LIST rmp2_dynamics_step_contacts_lists of one robot: the same routine, the
// robot's spheres being the table spheres [K][4] itself or the list_len records spheres[list[i]] of it (contact_list_span gives
// list and list_len from csr_offset / csr_index).  qlo / qhi: [n_dof] or both null (no limits).  contact_out [n_dof], lambda_out
// / pair_out [kMaxContacts]: null or the robot's rows.  lds / stride: room for contact_words(N) floats (with SelfPairs:
// contact_self_words(N)).  The spheres are scanned
// once, before the substeps: a non-finite record makes the robot NaN, an invalid list NaN with the status word
// RMP2_CONTACT_LIST_INVALID alone (its substeps run on no spheres, and nothing is read through its entries).  With Cy =
// CylinderList the robot's cylinder list is scanned in the same place, by the same rule and with the same status word.
template <int N, int SLOTS, bool LIST = false, class Pl = NoPlanes, class Cp = NoCapsules, class Sp = NoSelfPairs, class Cy = NoCylinders>
__host__ __device__ inline void dynamics_step_contacts_robot(const DevOp* ops, int n_ops, int n_dof, const float* inert,
                                                             const float base_acc[3], float* q_io, float* qd_io,
                                                             const float* u_in, bool accel, const float* lim, const float* qlo,
                                                             const float* qhi, const float* caps, const float* spheres, int K,
                                                             float d_act, float dt, int substeps, float* qdd_out, float* tau_out,
                                                             float* stop_out, float* contact_out, float* lambda_out,
                                                             int32_t* pair_out, uint32_t* status_out, float* lds, int stride,
                                                             const int32_t* list = nullptr, int list_len = 0, Pl pl = Pl{},
                                                             Cp oc = Cp{}, Sp sp = Sp{}, Cy cy = Cy{}) {
  auto src = contact_source<LIST>(spheres, K, list, list_len);
  float* Ms = lds;
  float* Jr = Ms + (size_t)fd_tri(N) * stride;
  float* Yw = Jr + (size_t)kMaxContacts * N * stride;
  float* Lw = Yw + (size_t)N * N * stride;
  float* mu = Lw + (size_t)fd_tri(N) * stride;
  if constexpr (Sp::kOn) sp.seg = Yw;   // (lds: room for contact_self_words(N) floats)
  float q[N], qd[N], u[N], qdd[N], tapp[N], stop[N], cont[N], lamc[kMaxContacts];
  int cidx[kMaxContacts];
  float poison = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[j] = j < n_dof ? q_io[j] : 0.f;
    qd[j] = j < n_dof ? qd_io[j] : 0.f;
    u[j] = j < n_dof ? u_in[j] : 0.f;
    poison += q[j] * 0.f + qd[j] * 0.f + u[j] * 0.f;
  }
  float table_poison = 0.f;   // a non-finite sphere record: every robot it belongs to NaN
  bool invalid = false;
  if constexpr (LIST) {
    table_poison = src.scan(invalid);
  } else {
    for (int s = 0; s < 4 * src.K; ++s) table_poison += src.spheres[s] * 0.f;
  }
  if constexpr (Pl::kOn) {   // a non-finite plane value: every robot NaN
    for (int s = 0; s < 4 * pl.P; ++s) table_poison += pl.planes[s] * 0.f;
  }
  if constexpr (Cp::kOn) {   // a non-finite capsule value: every robot NaN
    for (int s = 0; s < 8 * oc.C; ++s) table_poison += oc.capsules[s] * 0.f;
  }
  if constexpr (Cy::kList) {   // a non-finite value in a record of the robot's own list: that robot NaN; an invalid list as above
    bool cyl_invalid = false;
    table_poison += cy.scan(cyl_invalid);
    invalid = invalid || cyl_invalid;
  } else if constexpr (Cy::kOn) {   // a non-finite cylinder value: every robot NaN
    for (int s = 0; s < 8 * cy.Y; ++s) table_poison += cy.cylinders[s] * 0.f;
  }
  uint32_t status = 0u;
  int most = 0;
  for (int s = 0; s < substeps; ++s) {
    const uint32_t owned = fd_evaluate_saved<N, SLOTS>(ops, n_ops, n_dof, inert, base_acc, q, qd, u, accel, lim, qdd, tapp, Ms, stride);
    float vstar[N], lb[N], ub[N], v[N], cgap[kMaxContacts];
    uint32_t W = 0u, upper = 0u;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      vstar[j] = qd[j] + dt * qdd[j];
      lb[j] = -INFINITY;
      ub[j] = INFINITY;
      if (qlo && j < n_dof && ((owned >> j) & 1u)) {
        lb[j] = fminf((qlo[j] - q[j]) / dt, 0.f);
        ub[j] = fmaxf((qhi[j] - q[j]) / dt, 0.f);
      }
      const bool below = vstar[j] < lb[j], above = vstar[j] > ub[j];
      v[j] = below ? lb[j] : (above ? ub[j] : vstar[j]);
      if (below || above) W |= 1u << j;
      if (above) upper |= 1u << j;
      cont[j] = 0.f;
    }
    int excess = 0;
    const int nc = contact_candidates_from<N, SLOTS>(ops, n_ops, caps, src, d_act, q, Jr, stride, cgap, cidx, excess, pl, oc, sp, cy);
    if (excess > 0) status |= RMP2_CONTACT_OVERFLOW;
#pragma unroll
    for (int c = 0; c < kMaxContacts; ++c) lamc[c] = 0.f;
    if (nc == 0) {   // rmp2_joint_stops.h's substep, in its own words
      if (!W) {
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
    } else {
      float Ul[fd_tri(N)], cb[kMaxContacts];
#pragma unroll
      for (int k = 0; k < fd_tri(N); ++k) Ul[k] = Ms[k * stride];
      const bool ok = fd_cholesky<N>(Ul);
#pragma unroll
      for (int k = 0; k < fd_tri(N); ++k) Ms[k * stride] = Ul[k];
#pragma unroll
      for (int c = 0; c < kMaxContacts; ++c) cb[c] = -fmaxf(cgap[c], 0.f) / dt;
      bool capped;
      const int it = contacts_solve<N>(Ms, Jr, Yw, Lw, mu, stride, vstar, lb, ub, nc, cb, v, stop, lamc, capped);
      most = it > most ? it : most;
      bool any_stop = false, any_contact = false;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        any_stop = any_stop || stop[j] != 0.f;
        if (!ok) v[j] = stop[j] = NAN;
      }
#pragma unroll
      for (int c = 0; c < kMaxContacts; ++c) {
        any_contact = any_contact || lamc[c] > 0.f;
        if (c < nc) {
          const float l = ok ? lamc[c] : NAN;
          const float* row = Jr + (size_t)c * N * stride;
#pragma unroll
          for (int j = 0; j < N; ++j) cont[j] += l * row[j * stride];
          lamc[c] = l / dt;
        }
      }
      status |= (any_stop ? RMP2_STOP_ACTIVE : 0u) | (any_contact ? RMP2_CONTACT_ACTIVE : 0u) | (capped ? RMP2_STOP_CAPPED : 0u);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      qdd[j] += (v[j] - vstar[j]) / dt;
      stop[j] /= dt;
      cont[j] /= dt;
      qd[j] = v[j];
      const float q0 = q[j];
      float q1 = q0 + dt * v[j];
      if (qlo && j < n_dof && ((owned >> j) & 1u)) {
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
  const bool bad = !(poison == 0.f) || !(table_poison == 0.f) || invalid;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < n_dof) {
      q_io[j] = bad ? NAN : q[j];
      qd_io[j] = bad ? NAN : qd[j];
      if (qdd_out) qdd_out[j] = bad ? NAN : qdd[j];
      if (tau_out) tau_out[j] = bad ? NAN : tapp[j];
      if (stop_out) stop_out[j] = bad ? NAN : stop[j];
      if (contact_out) contact_out[j] = bad ? NAN : cont[j];
    }
#pragma unroll
  for (int c = 0; c < kMaxContacts; ++c) {
    if (lambda_out) lambda_out[c] = bad ? NAN : lamc[c];
    if (pair_out) pair_out[c] = bad ? -1 : cidx[c];
  }
  if (status_out) *status_out = invalid ? RMP2_CONTACT_LIST_INVALID : status | ((uint32_t)most << 8);
}

#if defined(__HIPCC__)
// The kernels: one lane per robot, one wave per block; the per-lane storage of the wave's 64 robots in LDS, lane-interleaved.
// Each keeps a parameter list of its own, scalars and __restrict__ pointers, and spells out the same twenty lines -- the rows, the
// base acceleration, the sphere list span, the call -- for measured reasons (profiles/contacts_fold_timing.json):
//  - one kernel over a by-value struct of all forms' arguments loses __restrict__ on the members; compiled for the cylinder units
//    it moved register allocation and the scalar loads throughout;
//  - a shared __device__ __forceinline__ lane body under these five parameter lists leaves every kernel's vector arithmetic,
//    registers and LDS what they are and gives the same bits, but the tests of the optional outputs then compile to scalar branches,
//    and on the MI355X the sphere, plane and self kernels ran 0.5 to 1.9 % slower, the cylinder and cylinder-list kernels over
//    sphere lists 0.3 to 1 % (the capsule kernels over sphere lists 2 % faster, the rest inside the spread).
//
// The sphere and plane forms.  LIST: every robot's own list over a shared pool (csr_offset / csr_index; the lanes' trip counts and
// sphere addresses differ), else the shared table and both are unused.  PLANES: planes [P][4] beside the spheres, read at uniform
// addresses, F the robot's frame count (the plane rows go into the same candidate slots: no word more); else the three are unused
// and the routines are instantiated with NoPlanes.
template <int N, int SLOTS, bool LIST, bool PLANES>
__global__ void __launch_bounds__(kWave)
rmp2_dynamics_step_contacts_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, float ax, float ay,
                                   float az, float* q, float* qd, const float* __restrict__ u, int accel,
                                   const float* __restrict__ lim, const float* __restrict__ qlo, const float* __restrict__ qhi,
                                   const float* __restrict__ caps, const float* __restrict__ spheres, int K,
                                   const int32_t* __restrict__ csr_offset, const int32_t* __restrict__ csr_index,
                                   const float* __restrict__ planes, int P, int F, float d_act, float dt, int substeps,
                                   float* __restrict__ qdd_out, float* __restrict__ tau_out, float* __restrict__ stop_out,
                                   float* __restrict__ contact_out, float* __restrict__ lambda_out,
                                   int32_t* __restrict__ pair_out, uint32_t* __restrict__ status_out, int R) {
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
  using Pl = std::conditional_t<PLANES, PlaneTable, NoPlanes>;
  Pl pl{};
  if constexpr (PLANES) pl = {planes, P, F};
  dynamics_step_contacts_robot<N, SLOTS, LIST, Pl>(
      prog->ops, prog->n_ops, n_dof, inert, base_acc, q + row, qd + row, u + row, accel != 0, lim, qlo, qhi, caps, spheres, K, d_act,
      dt, substeps, qdd_out ? qdd_out + row : nullptr, tau_out ? tau_out + row : nullptr, stop_out ? stop_out + row : nullptr,
      contact_out ? contact_out + row : nullptr, lambda_out ? lambda_out + crow : nullptr, pair_out ? pair_out + crow : nullptr,
      status_out ? status_out + robot : nullptr, lds + threadIdx.x, kWave, list, len, pl);
}

// The capsule forms (rmp2_dynamics_step_contacts_capsules): planes AND capsules on.  capsules [C][8] beside the planes; P == 0 and
// C == 0 run it too.
template <int N, int SLOTS, bool LIST>
__global__ void __launch_bounds__(kWave)
rmp2_dynamics_step_contacts_capsules_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, float ax, float ay,
                                            float az, float* q, float* qd, const float* __restrict__ u, int accel,
                                            const float* __restrict__ lim, const float* __restrict__ qlo,
                                            const float* __restrict__ qhi, const float* __restrict__ caps,
                                            const float* __restrict__ spheres, int K, const int32_t* __restrict__ csr_offset,
                                            const int32_t* __restrict__ csr_index, const float* __restrict__ planes, int P,
                                            const float* __restrict__ capsules, int C, int F, float d_act, float dt, int substeps,
                                            float* __restrict__ qdd_out, float* __restrict__ tau_out, float* __restrict__ stop_out,
                                            float* __restrict__ contact_out, float* __restrict__ lambda_out,
                                            int32_t* __restrict__ pair_out, uint32_t* __restrict__ status_out, int R) {
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
  dynamics_step_contacts_robot<N, SLOTS, LIST, PlaneTable, CapsuleTable>(
      prog->ops, prog->n_ops, n_dof, inert, base_acc, q + row, qd + row, u + row, accel != 0, lim, qlo, qhi, caps, spheres, K, d_act,
      dt, substeps, qdd_out ? qdd_out + row : nullptr, tau_out ? tau_out + row : nullptr, stop_out ? stop_out + row : nullptr,
      contact_out ? contact_out + row : nullptr, lambda_out ? lambda_out + crow : nullptr, pair_out ? pair_out + crow : nullptr,
      status_out ? status_out + robot : nullptr, lds + threadIdx.x, kWave, list, len, PlaneTable{planes, P, F},
      CapsuleTable{capsules, C, F, P});
}

// The self forms (rmp2_dynamics_step_contacts_self): planes, capsules AND self pairs on.  self_slot / self_begin / self_rec: the
// handle's pair tables (SelfPairs), n_self pairs; n_self == 0 reads none of them.
template <int N, int SLOTS, bool LIST>
__global__ void __launch_bounds__(kWave)
rmp2_dynamics_step_contacts_self_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, float ax, float ay,
                                        float az, float* q, float* qd, const float* __restrict__ u, int accel,
                                        const float* __restrict__ lim, const float* __restrict__ qlo,
                                        const float* __restrict__ qhi, const float* __restrict__ caps,
                                        const float* __restrict__ spheres, int K, const int32_t* __restrict__ csr_offset,
                                        const int32_t* __restrict__ csr_index, const float* __restrict__ planes, int P,
                                        const float* __restrict__ capsules, int C, const int32_t* __restrict__ self_slot,
                                        const int32_t* __restrict__ self_begin, const int32_t* __restrict__ self_rec, int n_self,
                                        int F, float d_act, float dt, int substeps, float* __restrict__ qdd_out,
                                        float* __restrict__ tau_out, float* __restrict__ stop_out, float* __restrict__ contact_out,
                                        float* __restrict__ lambda_out, int32_t* __restrict__ pair_out,
                                        uint32_t* __restrict__ status_out, int R) {
  static_assert(contact_self_words(N) * kWave * sizeof(float) <= 65536, "the per-lane storage of one wave must fit 64 KiB of LDS");
  __shared__ float lds[contact_self_words(N) * kWave];
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
  dynamics_step_contacts_robot<N, SLOTS, LIST, PlaneTable, CapsuleTable, SelfPairs>(
      prog->ops, prog->n_ops, n_dof, inert, base_acc, q + row, qd + row, u + row, accel != 0, lim, qlo, qhi, caps, spheres, K, d_act,
      dt, substeps, qdd_out ? qdd_out + row : nullptr, tau_out ? tau_out + row : nullptr, stop_out ? stop_out + row : nullptr,
      contact_out ? contact_out + row : nullptr, lambda_out ? lambda_out + crow : nullptr, pair_out ? pair_out + crow : nullptr,
      status_out ? status_out + robot : nullptr, lds + threadIdx.x, kWave, list, len, PlaneTable{planes, P, F},
      CapsuleTable{capsules, C, F, P}, SelfPairs{self_slot, self_begin, self_rec, n_self, F, nullptr});
}

// The cylinder forms (rmp2_dynamics_step_contacts_cylinders): planes, capsules, self pairs AND the cylinder table on.  cylinders
// [Y][8] (CylinderTable); Y == 0 reads nothing of it.  n_self == 0 (no pairs set, or the call's self_pairs flag 0) reads none of the
// pair tables.  No LDS beyond the self forms'.
template <int N, int SLOTS, bool LIST>
__global__ void __launch_bounds__(kWave)
rmp2_dynamics_step_contacts_cylinders_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, float ax, float ay,
                                             float az, float* q, float* qd, const float* __restrict__ u, int accel,
                                             const float* __restrict__ lim, const float* __restrict__ qlo,
                                             const float* __restrict__ qhi, const float* __restrict__ caps,
                                             const float* __restrict__ spheres, int K, const int32_t* __restrict__ csr_offset,
                                             const int32_t* __restrict__ csr_index, const float* __restrict__ planes, int P,
                                             const float* __restrict__ capsules, int C, const int32_t* __restrict__ self_slot,
                                             const int32_t* __restrict__ self_begin, const int32_t* __restrict__ self_rec,
                                             int n_self, const float* __restrict__ cylinders, int Y, int F, float d_act, float dt,
                                             int substeps, float* __restrict__ qdd_out, float* __restrict__ tau_out,
                                             float* __restrict__ stop_out, float* __restrict__ contact_out,
                                             float* __restrict__ lambda_out, int32_t* __restrict__ pair_out,
                                             uint32_t* __restrict__ status_out, int R) {
  static_assert(contact_self_words(N) * kWave * sizeof(float) <= 65536, "the per-lane storage of one wave must fit 64 KiB of LDS");
  __shared__ float lds[contact_self_words(N) * kWave];
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
  dynamics_step_contacts_robot<N, SLOTS, LIST, PlaneTable, CapsuleTable, SelfPairs, CylinderTable>(
      prog->ops, prog->n_ops, n_dof, inert, base_acc, q + row, qd + row, u + row, accel != 0, lim, qlo, qhi, caps, spheres, K, d_act,
      dt, substeps, qdd_out ? qdd_out + row : nullptr, tau_out ? tau_out + row : nullptr, stop_out ? stop_out + row : nullptr,
      contact_out ? contact_out + row : nullptr, lambda_out ? lambda_out + crow : nullptr, pair_out ? pair_out + crow : nullptr,
      status_out ? status_out + robot : nullptr, lds + threadIdx.x, kWave, list, len, PlaneTable{planes, P, F},
      CapsuleTable{capsules, C, F, P}, SelfPairs{self_slot, self_begin, self_rec, n_self, F, nullptr},
      CylinderTable{cylinders, Y, F, P, C});
}

// The cylinder-list forms (rmp2_dynamics_step_contacts_cylinder_lists): the cylinder forms with every robot's own list over the
// pool cylinders [Y][8] (CylinderList; cyl_offset / cyl_index laid out as csr_offset / csr_index).  LIST: the spheres' form, as
// everywhere.  No LDS beyond the self forms'.
template <int N, int SLOTS, bool LIST>
__global__ void __launch_bounds__(kWave)
rmp2_dynamics_step_contacts_cylinder_lists_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, float ax,
                                                  float ay, float az, float* q, float* qd, const float* __restrict__ u, int accel,
                                                  const float* __restrict__ lim, const float* __restrict__ qlo,
                                                  const float* __restrict__ qhi, const float* __restrict__ caps,
                                                  const float* __restrict__ spheres, int K, const int32_t* __restrict__ csr_offset,
                                                  const int32_t* __restrict__ csr_index, const float* __restrict__ planes, int P,
                                                  const float* __restrict__ capsules, int C, const int32_t* __restrict__ self_slot,
                                                  const int32_t* __restrict__ self_begin, const int32_t* __restrict__ self_rec,
                                                  int n_self, const float* __restrict__ cylinders, int Y,
                                                  const int32_t* __restrict__ cyl_offset, const int32_t* __restrict__ cyl_index,
                                                  int F, float d_act, float dt, int substeps, float* __restrict__ qdd_out,
                                                  float* __restrict__ tau_out, float* __restrict__ stop_out,
                                                  float* __restrict__ contact_out, float* __restrict__ lambda_out,
                                                  int32_t* __restrict__ pair_out, uint32_t* __restrict__ status_out, int R) {
  static_assert(contact_self_words(N) * kWave * sizeof(float) <= 65536, "the per-lane storage of one wave must fit 64 KiB of LDS");
  __shared__ float lds[contact_self_words(N) * kWave];
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
  int cyl_beg;
  const int cyl_len = contact_list_span(cyl_offset, robot, cyl_beg);   // (-1: no list; above the cap: as it is -- scan refuses both)
  dynamics_step_contacts_robot<N, SLOTS, LIST, PlaneTable, CapsuleTable, SelfPairs, CylinderList>(
      prog->ops, prog->n_ops, n_dof, inert, base_acc, q + row, qd + row, u + row, accel != 0, lim, qlo, qhi, caps, spheres, K, d_act,
      dt, substeps, qdd_out ? qdd_out + row : nullptr, tau_out ? tau_out + row : nullptr, stop_out ? stop_out + row : nullptr,
      contact_out ? contact_out + row : nullptr, lambda_out ? lambda_out + crow : nullptr, pair_out ? pair_out + crow : nullptr,
      status_out ? status_out + robot : nullptr, lds + threadIdx.x, kWave, list, len, PlaneTable{planes, P, F},
      CapsuleTable{capsules, C, F, P}, SelfPairs{self_slot, self_begin, self_rec, n_self, F, nullptr},
      CylinderList{cylinders, Y, cyl_index + cyl_beg, cyl_len, F, P, C});
}
#endif

}  // namespace rmp2

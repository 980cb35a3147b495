// rmp2_stages.h -- the geometry stage kernels of rmp2_hip.hip (the only file that includes this one): FK of all frames, the
// closest-point stage in its two forms, the self-pair stage, the two hull stages and FK differentiation of one frame, with the
// pieces they share:
//   walk_frames           the position walk of a DevProgram (restore from a save slot, visit_frame<false>, save): FK, the wave
//                         form of the closest-point stage, the hull stage
//   link_segment_world    a link capsule's end points taken to the base frame
//   obstacle_pair_points  the closed form of an obstacle pair (wave form of the closest-point stage, obstacle half of the self stage)
//   q_is_non_finite       the non-finite-q probe of the hull stages
//   store_hull_pair       the write-back of a hull hit (point leaf / distance leaf), over one row layout of the leaf frame
// Walks that are NOT on walk_frames, and why (profiles/stage_walker_ab.txt has the measurements):
//   rmp2_diff_kernel (below) and rmp2_step_kernel (rmp2_hip.hip) carry velocities (visit_frame<true>, qd) and store the joint axis
//   z between the visit and the save; the diff kernel also leaves the kernel from inside the walk, which a visitor could only do
//   through a flag of its own.
//   rmp2_self_hull_stage_kernel's walk is select-based (walk_frame_position): branch-free on purpose, so that the kernel needs no
//   scratch.
//   rmp2_closest_kernel (the RMP2_KERNEL=lane form) keeps its written-out walk for its bits, rmp2_self_stage_kernel its two for
//   its speed; see there.
#pragma once
#include "rmp2_device.h"
#include "rmp2_hull.h"

namespace {   // (unnamed and outside rmp2, as in rmp2_hip.hip before: the kernels keep their symbol names)

using namespace rmp2;

// The position walk: visitor(op, cur) sees every frame of the program in order, after the frame's state went to its save slot.
template <int SLOTS, class Visitor>
__device__ __forceinline__ void walk_frames(const DevProgram* __restrict__ prog, const float* __restrict__ my_q, const Visitor& visitor) {
  FrameState cur;
  FrameState slot[SLOTS > 0 ? SLOTS : 1];
  for (int k = 0; k < prog->n_ops; ++k) {
    const DevOp& op = prog->ops[k];
    if (SLOTS > 0 && op.restore >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.restore == s) cur = slot[s];
    }
    float z[3];
    visit_frame<false>(cur, op, op.qidx >= 0 ? my_q[op.qidx] : 0.f, 0.f, op.restore == -2, z);
    if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.save == s) slot[s] = cur;
    }
    visitor(op, static_cast<const FrameState&>(cur));
  }
}

// A link capsule (a, radius, b) in its frame's own coordinates -> its end points in the base frame, the radius in a.w.
__device__ __forceinline__ void link_segment_world(const FrameState& cur, const float* cap8, float4& a, float4& b) {
  float A[3], B[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    A[i] = cur.p[i] + cur.R[3 * i] * cap8[0] + cur.R[3 * i + 1] * cap8[1] + cur.R[3 * i + 2] * cap8[2];
    B[i] = cur.p[i] + cur.R[3 * i] * cap8[4] + cur.R[3 * i + 1] * cap8[5] + cur.R[3 * i + 2] * cap8[6];
  }
  a = make_float4(A[0], A[1], A[2], cap8[3]);
  b = make_float4(B[0], B[1], B[2], 0.f);
}

// true when some q[j] is NaN or Inf
__device__ __forceinline__ bool q_is_non_finite(const float* my_q, int n_dof) {
  float qz = 0.f;
  for (int j = 0; j < n_dof; ++j) qz += 0.f * my_q[j];
  return !(qz == 0.f);
}

// =========================================================================================
// device: FK of all frames
// =========================================================================================
template <int SLOTS>
__global__ void __launch_bounds__(kWave)
rmp2_fk_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ q, float* __restrict__ T, int R) {
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  const int n_dof = prog->n_dof, F = prog->n_frames;
  walk_frames<SLOTS>(prog, q + (size_t)robot * n_dof, [&](const DevOp& op, const FrameState& cur) {
    float* o = T + ((size_t)robot * F + op.frame) * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) o[4 * i + j] = cur.R[3 * i + j];
      o[4 * i + 3] = cur.p[i];
    }
    o[12] = o[13] = o[14] = 0.f;
    o[15] = 1.f;
  });
}

// Closest-point stage on its own: control point = frame origin of each distance leaf, nearest surface
// point of every primitive of the shared table (simulation.py:462-484 calculate_distances; lane per robot).
// The walk is written out here: on walk_frames the compiler contracts the three-term sums of the frame-origin branch (|diff|^2,
// capsule_centre's dot products) around another product, and p_obs moves in its last bit for spheres and capsules.
template <int SLOTS>
__global__ void __launch_bounds__(kWave)
rmp2_closest_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ q, const ObsArgs obs,
                    const float* __restrict__ link_caps, float* __restrict__ p_link, float* __restrict__ p_obs, int R) {
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  const float* my_q = q + (size_t)robot * prog->n_dof;
  FrameState cur;
  FrameState slot[SLOTS > 0 ? SLOTS : 1];
  for (int k = 0; k < prog->n_ops; ++k) {
    const DevOp& op = prog->ops[k];
    if (SLOTS > 0 && op.restore >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.restore == s) cur = slot[s];
    }
    float z[3];
    visit_frame<false>(cur, op, op.qidx >= 0 ? my_q[op.qidx] : 0.f, 0.f, op.restore == -2, z);
    if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.save == s) slot[s] = cur;
    }
    for (int li = 0; li < op.leaf_count; ++li) {
      const DevLeaf& lf = prog->leaves[prog->fk_leaves[op.leaf_begin + li]];
      if (lf.taskmap != RMP2_TASKMAP_FK_DISTANCE) continue;
      const size_t base = ((size_t)robot * obs.n_pairs + obs.pair_begin[lf.index]) * 3;
      if (link_caps) {
        // link geometry: the leaf's link as a capsule (a, radius, b) in the frame's own coordinates; per pair the nearest
        // points of the link capsule and the obstacle primitive (their surfaces), as PyBullet reports them for the link's
        // collision shape (simulation.py:462-484 -> data_management.py:22-37)
        float4 la, lb;
        link_segment_world(cur, link_caps + 8 * (obs.pair_begin[lf.index] / obs.n_spheres), la, lb);  // ordinal of the distance leaf
        const float A[3] = {la.x, la.y, la.z}, B[3] = {lb.x, lb.y, lb.z};
        const float r_link = la.w;
        for (int b = 0; b < obs.n_spheres; ++b) {
          if (obs.cylinder) {  // link capsule against a finite cylinder: nearest points by bisection on the convex distance
            const float4 ca = reinterpret_cast<const float4*>(obs.spheres)[2 * b];
            const float4 cb = reinterpret_cast<const float4*>(obs.spheres)[2 * b + 1];
            const float Dl[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
            float X[3], Y[3], n[3], sd;
            segment_cylinder(ca, cb, A, Dl, X, Y, n, sd);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              p_link[base + 3 * b + c] = X[c] - r_link * n[c];
              p_obs[base + 3 * b + c] = Y[c];
            }
            continue;
          }
          float C[3], D[3], r_obs;
          if (obs.capsule) {
            const float4 ca = reinterpret_cast<const float4*>(obs.spheres)[2 * b];
            const float4 cb = reinterpret_cast<const float4*>(obs.spheres)[2 * b + 1];
            C[0] = ca.x, C[1] = ca.y, C[2] = ca.z, D[0] = cb.x, D[1] = cb.y, D[2] = cb.z, r_obs = ca.w;
          } else {
            const float4 sp = reinterpret_cast<const float4*>(obs.spheres)[b];
            C[0] = D[0] = sp.x, C[1] = D[1] = sp.y, C[2] = D[2] = sp.z, r_obs = sp.w;
          }
          float sl, to;
          segment_segment(A, B, C, D, sl, to);
          float X[3], Y[3], n[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            X[c] = A[c] + sl * (B[c] - A[c]);
            Y[c] = C[c] + to * (D[c] - C[c]);
            n[c] = X[c] - Y[c];
          }
          const float dn = link_normal_length(n);  // (intersecting axes: n = +z, dn = 1)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float u = n[c] / dn;
            p_link[base + 3 * b + c] = X[c] - r_link * u;
            p_obs[base + 3 * b + c] = Y[c] + r_obs * u;
          }
        }
        continue;
      }
      for (int b = 0; b < obs.n_spheres; ++b) {
        float4 sp;
        float ctr[3];
        if (obs.cylinder) {  // frame origin against a finite cylinder: its nearest surface point
          float Y[3], n[3], sd;
          point_cylinder(reinterpret_cast<const float4*>(obs.spheres)[2 * b], reinterpret_cast<const float4*>(obs.spheres)[2 * b + 1], cur.p, Y, n, sd);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            p_link[base + 3 * b + c] = cur.p[c];
            p_obs[base + 3 * b + c] = Y[c];
          }
          continue;
        }
        if (obs.capsule) {
          sp = reinterpret_cast<const float4*>(obs.spheres)[2 * b];
          capsule_centre(sp, reinterpret_cast<const float4*>(obs.spheres)[2 * b + 1], cur.p, ctr);
        } else {
          sp = reinterpret_cast<const float4*>(obs.spheres)[b];
          ctr[0] = sp.x, ctr[1] = sp.y, ctr[2] = sp.z;
        }
        const float diff[3] = {cur.p[0] - ctr[0], cur.p[1] - ctr[1], cur.p[2] - ctr[2]};
        const float dc = sqrtf(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          p_link[base + 3 * b + c] = cur.p[c];
          p_obs[base + 3 * b + c] = ctr[c] + sp.w * (diff[c] / dc);
        }
      }
    }
  }
}

// The same stage with coalesced output (the arrays are the whole cost: 24 B per pair, 6 KB per robot at 8 x 32 pairs).
// One wave per kClosestRobots robots.  Phase 1, a lane per robot: FK, and each distance leaf's link segment in world
// coordinates (A, r_link, B -- A = B = the frame origin, r_link = 0 without link geometry) into LDS.  Phase 2, a lane per PAIR:
// the lane keeps its obstacle primitive in registers and walks the wave's robots; the 64 lanes of a chunk write 64 consecutive
// pairs of one robot, 768 contiguous bytes per array and store, past the cache (written once, read by a later kernel).  The
// lane-per-robot kernel above writes 4 bytes per lane at a 3 KB stride: 1.2 TB/s, 325 us for 65 536 robots x 256 pairs; this
// one 4.1-4.9 TB/s, 82-98 us (a memset of the same bytes: 6.5 TB/s).  Same closed forms; the unit normal is scaled by one
// reciprocal instead of three divisions, and a sphere obstacle takes the point-segment form of segment_segment.
constexpr int kClosestRobots = 16;
typedef float f32x3 __attribute__((ext_vector_type(3), aligned(4)));

// Phase 2's closed form of one obstacle pair: link segment (sa, sb; radius in sa.w; LINK = false: the frame origin sa alone)
// against the obstacle (ca, cb; radius in ca.w; CAPS = false: the sphere ca alone) -> the two surface points.
template <bool LINK, bool CAPS>
__device__ __forceinline__ void obstacle_pair_points(const float4 sa, const float4 sb, const float4 ca, const float4 cb,
                                                     f32x3& p_link3, f32x3& p_obs3) {
  const float r_obs = ca.w;
  float X[3] = {sa.x, sa.y, sa.z}, Y[3] = {ca.x, ca.y, ca.z};  // nearest points of the two axes
  if (LINK) {
    const float A[3] = {sa.x, sa.y, sa.z}, B[3] = {sb.x, sb.y, sb.z};
    const float C[3] = {ca.x, ca.y, ca.z}, D[3] = {cb.x, cb.y, cb.z};
    float sl, to = 0.f;
    if (CAPS) {
      segment_segment(A, B, C, D, sl, to);
    } else {  // (segment_segment with a point as the second segment)
      const float d1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
      const float rr[3] = {A[0] - C[0], A[1] - C[1], A[2] - C[2]};
      const float aa = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
      const float cc = d1[0] * rr[0] + d1[1] * rr[1] + d1[2] * rr[2];
      sl = aa > 0.f ? fminf(fmaxf(-cc / aa, 0.f), 1.f) : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      X[c] = A[c] + sl * (B[c] - A[c]);
      if (CAPS) Y[c] = C[c] + to * (D[c] - C[c]);
    }
  } else if (CAPS) {
    capsule_centre(ca, cb, X, Y);
  }
  float n[3] = {X[0] - Y[0], X[1] - Y[1], X[2] - Y[2]};
  // (link geometry: intersecting axes take the fixed normal +z; a frame origin ON a centre is the reference's own 0 / 0)
  const float inv = 1.0f / (LINK ? link_normal_length(n) : sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]));
  const float wl = LINK ? sa.w * inv : 0.f, wo = r_obs * inv;
  p_link3 = f32x3{X[0] - wl * n[0], X[1] - wl * n[1], X[2] - wl * n[2]};
  p_obs3 = f32x3{Y[0] + wo * n[0], Y[1] + wo * n[1], Y[2] + wo * n[2]};
}

template <int SLOTS, bool LINK, bool CAPS>
__global__ void __launch_bounds__(kWave)
rmp2_closest_wave_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ q, const ObsArgs obs,
                         const float* __restrict__ link_caps, int n_dist, float* __restrict__ p_link, float* __restrict__ p_obs,
                         int R) {
  extern __shared__ float4 seg[];  // [kClosestRobots][n_dist][2] = (A, r_link), (B, -)
  const int lane = threadIdx.x;
  const int r0 = blockIdx.x * kClosestRobots;
  const int robot = r0 + lane;
  if (lane < kClosestRobots && robot < R) {
    walk_frames<SLOTS>(prog, q + (size_t)robot * prog->n_dof, [&](const DevOp& op, const FrameState& cur) {
      for (int li = 0; li < op.leaf_count; ++li) {
        const DevLeaf& lf = prog->leaves[prog->fk_leaves[op.leaf_begin + li]];
        if (lf.taskmap != RMP2_TASKMAP_FK_DISTANCE) continue;
        const int ord = obs.pair_begin[lf.index] / obs.n_spheres;  // ordinal of the distance leaf
        float4 a = make_float4(cur.p[0], cur.p[1], cur.p[2], 0.f), b = a;
        if (LINK) link_segment_world(cur, link_caps + 8 * ord, a, b);
        seg[(lane * n_dist + ord) * 2] = a;
        seg[(lane * n_dist + ord) * 2 + 1] = b;
      }
    });
  }
  __syncthreads();
  const int n_live = min(kClosestRobots, R - r0);
  const int P = obs.n_pairs, K = obs.n_spheres;
  for (int p0 = 0; p0 < P; p0 += kWave) {
    const int p = p0 + lane;
    const bool ok = p < P;
    const int pp = ok ? p : 0;
    const int leaf = pp / K, bi = pp - leaf * K;
    float4 ca, cb;
    if (CAPS) {
      ca = reinterpret_cast<const float4*>(obs.spheres)[2 * bi];
      cb = reinterpret_cast<const float4*>(obs.spheres)[2 * bi + 1];
    } else {
      ca = cb = reinterpret_cast<const float4*>(obs.spheres)[bi];
    }
    size_t off = ((size_t)r0 * P + p) * 3;
    for (int r = 0; r < n_live; ++r, off += (size_t)P * 3) {
      const float4 sa = seg[(r * n_dist + leaf) * 2];
      if (CAPS && obs.cylinder) {  // (wave-uniform) finite cylinders: nearest SURFACE point and outward normal (rmp2_device.h)
        float Xc[3] = {sa.x, sa.y, sa.z}, Yc[3], nc[3], sd;
        if (LINK) {
          const float4 sb = seg[(r * n_dist + leaf) * 2 + 1];
          const float Al[3] = {sa.x, sa.y, sa.z}, Dl[3] = {sb.x - sa.x, sb.y - sa.y, sb.z - sa.z};
          segment_cylinder(ca, cb, Al, Dl, Xc, Yc, nc, sd);
        } else {
          point_cylinder(ca, cb, Xc, Yc, nc, sd);
        }
        if (ok) {
          const float wl = LINK ? sa.w : 0.f;
          __builtin_nontemporal_store(f32x3{Xc[0] - wl * nc[0], Xc[1] - wl * nc[1], Xc[2] - wl * nc[2]}, reinterpret_cast<f32x3*>(p_link + off));
          __builtin_nontemporal_store(f32x3{Yc[0], Yc[1], Yc[2]}, reinterpret_cast<f32x3*>(p_obs + off));
        }
        continue;
      }
      f32x3 pl3, po3;
      obstacle_pair_points<LINK, CAPS>(sa, LINK ? seg[(r * n_dist + leaf) * 2 + 1] : sa, ca, cb, pl3, po3);
      if (ok) {
        __builtin_nontemporal_store(pl3, reinterpret_cast<f32x3*>(p_link + off));
        __builtin_nontemporal_store(po3, reinterpret_cast<f32x3*>(p_obs + off));
      }
    }
  }
}

// ---- self collision (include/rmp2.h rmp2_set_self_collision) ---------------------------------------------------------------
// The pair list of a handle, compiled by rmp2_set_self_collision.  "Pair leaves" are the leaves that take per-pair obstacle data
// (FK_DISTANCE and FK_POINT), numbered in descriptor order (the ordinal); B slots are the distinct links that appear as B.
struct SelfProg {
  int32_t n_leaves;                          // pair leaves L
  int32_t n_b;                               // B slots
  int32_t n_pairs;                           // S = self pairs per robot
  int32_t base_slot;                         // B slot of the base link, -1: none
  int32_t n_dist;                            // FK_DISTANCE leaves (rows of the obstacle stage's link segments)
  int32_t pad_[3];
  int32_t ord_of_leaf[RMP2_MAX_LEAVES];      // descriptor leaf -> pair-leaf ordinal, -1: not a pair leaf
  int32_t dord[RMP2_MAX_LEAVES];             // ordinal -> FK_DISTANCE ordinal (obstacle rows), -1: attached-point leaf
  int32_t self_begin[RMP2_MAX_LEAVES + 1];   // ordinal -> first self pair (prefix sums of S_l)
  int32_t b_slot_of_frame[RMP2_MAX_FRAMES];  // frame -> B slot, -1: the frame is no B link (the marker of the B walk)
  int32_t pair_b[RMP2_MAX_SELF_PAIRS];       // self pair -> B slot
  float leaf_cap[RMP2_MAX_LEAVES][8];        // ordinal -> capsule of the leaf's link in its frame coordinates
  float b_cap[RMP2_MAX_FRAMES + 1][8];       // B slot -> capsule in its frame coordinates (the base: base coordinates)
};

// Float4 records per robot in the stage's LDS: obstacle segments (2 per FK_DISTANCE leaf, only with a table), self segments
// (2 per pair leaf), the frame of each pair leaf (3: rows of R with the origin in .w), B segments (2 per B slot).
__host__ __device__ inline int self_lds_records(int n_dist_obs, int n_leaves, int n_b) { return 2 * n_dist_obs + 5 * n_leaves + 2 * n_b; }

// The self-pair stage (with the obstacle pairs of a shared table when OBS): one wave per nr = kClosestRobots robots, as
// rmp2_closest_wave_kernel.  Phase 1, a lane per robot: a walk of the step's program (`prog`: the pair leaves' frames, exactly the
// FK the obstacle stage computes) puts each pair leaf's link segment, its frame, and -- OBS -- the obstacle stage's segment of each
// distance leaf into LDS; a second walk, of the unpruned program (`prog_full`: leaf-less frames are not in the step's), puts the
// segment of every frame the B marker names.  Phase 2, a lane per pair: leaf l's range is [K obstacle pairs | S_l self pairs]
// (K = 0 without a table and for attached-point leaves); a chunk of 64 lanes writes 64 consecutive pairs of one robot per store.
// Obstacle pairs: rmp2_closest_wave_kernel's obstacle_pair_points.  Self pairs: rmp2_device.h link_pair_fields (the crossing
// guard keeps intersecting axes finite).  The two walks and the stage's own two link segments are written out, so that the
// table-less build compiles to the code it had before the stages shared pieces (instruction for instruction): with both walks in
// one body the compiler lays the leaf loop out once per save path, on walk_frames it does not, and rmp2_self_pairs then took
// 74.4 us instead of 72.6 us for config 3 at 65 536 robots, three runs of each build apart.
template <int SLOTS, bool OBS, bool LINK, bool CAPS>
__global__ void __launch_bounds__(kWave)
rmp2_self_stage_kernel(const DevProgram* __restrict__ prog, const DevProgram* __restrict__ prog_full, const SelfProg* __restrict__ sp,
                       const float* __restrict__ q, const ObsArgs obs, const float* __restrict__ link_caps, float* __restrict__ p_link,
                       float* __restrict__ p_obs, float* __restrict__ dist, int P, int R, int nr) {
  extern __shared__ float4 lds[];
  const int L = sp->n_leaves, NB = sp->n_b, ND = OBS ? sp->n_dist : 0, K = OBS ? obs.n_spheres : 0;
  const int W = self_lds_records(ND, L, NB);
  const int o_self = 2 * ND, o_rot = o_self + 2 * L, o_b = o_rot + 3 * L;   // record offsets inside a robot's W records
  const int lane = threadIdx.x;
  const int r0 = blockIdx.x * nr;
  const int robot = r0 + lane;
  if (lane < nr && robot < R) {
    float4* my = lds + (size_t)lane * W;
    const float* my_q = q + (size_t)robot * prog->n_dof;
    FrameState cur;
    FrameState slot[SLOTS > 0 ? SLOTS : 1];
    for (int k = 0; k < prog->n_ops; ++k) {
      const DevOp& op = prog->ops[k];
      if (SLOTS > 0 && op.restore >= 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
          if (op.restore == s) cur = slot[s];
      }
      float z[3];
      visit_frame<false>(cur, op, op.qidx >= 0 ? my_q[op.qidx] : 0.f, 0.f, op.restore == -2, z);
      if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
          if (op.save == s) slot[s] = cur;
      }
      for (int li = 0; li < op.leaf_count; ++li) {
        const DevLeaf& lf = prog->leaves[prog->fk_leaves[op.leaf_begin + li]];
        const int o = sp->ord_of_leaf[lf.index];
        if (o < 0) continue;
        if (OBS && lf.taskmap == RMP2_TASKMAP_FK_DISTANCE) {   // (rmp2_closest_wave_kernel's segment of the leaf)
          const int ord = sp->dord[o];
          float4 a = make_float4(cur.p[0], cur.p[1], cur.p[2], 0.f), b = a;
          if (LINK) link_segment_world(cur, link_caps + 8 * ord, a, b);
          my[2 * ord] = a;
          my[2 * ord + 1] = b;
        }
        const float* lc = sp->leaf_cap[o];
        float A[3], B[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          A[i] = cur.p[i] + cur.R[3 * i] * lc[0] + cur.R[3 * i + 1] * lc[1] + cur.R[3 * i + 2] * lc[2];
          B[i] = cur.p[i] + cur.R[3 * i] * lc[4] + cur.R[3 * i + 1] * lc[5] + cur.R[3 * i + 2] * lc[6];
        }
        my[o_self + 2 * o] = make_float4(A[0], A[1], A[2], lc[3]);
        my[o_self + 2 * o + 1] = make_float4(B[0], B[1], B[2], 0.f);
#pragma unroll
        for (int i = 0; i < 3; ++i) my[o_rot + 3 * o + i] = make_float4(cur.R[3 * i], cur.R[3 * i + 1], cur.R[3 * i + 2], cur.p[i]);
      }
    }
    // the B links: the unpruned walk, a segment for every marked frame
    for (int k = 0; k < prog_full->n_ops; ++k) {
      const DevOp& op = prog_full->ops[k];
      if (SLOTS > 0 && op.restore >= 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
          if (op.restore == s) cur = slot[s];
      }
      float z[3];
      visit_frame<false>(cur, op, op.qidx >= 0 ? my_q[op.qidx] : 0.f, 0.f, op.restore == -2, z);
      if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
          if (op.save == s) slot[s] = cur;
      }
      const int b = sp->b_slot_of_frame[op.frame];
      if (b < 0) continue;
      const float* bc = sp->b_cap[b];
      float A[3], B[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        A[i] = cur.p[i] + cur.R[3 * i] * bc[0] + cur.R[3 * i + 1] * bc[1] + cur.R[3 * i + 2] * bc[2];
        B[i] = cur.p[i] + cur.R[3 * i] * bc[4] + cur.R[3 * i + 1] * bc[5] + cur.R[3 * i + 2] * bc[6];
      }
      my[o_b + 2 * b] = make_float4(A[0], A[1], A[2], bc[3]);
      my[o_b + 2 * b + 1] = make_float4(B[0], B[1], B[2], 0.f);
    }
    if (sp->base_slot >= 0) {   // the fixed base: its capsule is in base coordinates already
      const float* bc = sp->b_cap[sp->base_slot];
      my[o_b + 2 * sp->base_slot] = make_float4(bc[0], bc[1], bc[2], bc[3]);
      my[o_b + 2 * sp->base_slot + 1] = make_float4(bc[4], bc[5], bc[6], 0.f);
    }
  }
  __syncthreads();
  const int n_live = min(nr, R - r0);
  for (int p0 = 0; p0 < P; p0 += kWave) {
    const int p = p0 + lane;
    const bool ok = p < P;
    // which leaf range the pair falls in, and which half of it
    int o = 0, begin = 0, kl = 0;
    for (int t = 0; t < L; ++t) {
      const int kt = (OBS && sp->dord[t] >= 0) ? K : 0;
      const int len = kt + sp->self_begin[t + 1] - sp->self_begin[t];
      if (p >= begin + len) {
        begin += len;
        continue;
      }
      o = t, kl = kt;
      break;
    }
    const int i = (ok ? p : begin) - begin;
    const bool is_obs = OBS && i < kl;
    const int bi = is_obs ? i : 0;
    const int j = is_obs ? 0 : min(sp->self_begin[o] + (i - kl), RMP2_MAX_SELF_PAIRS - 1);
    const int bslot = ok ? sp->pair_b[j] : 0;
    const bool point = sp->dord[o] < 0;
    const int leaf = OBS ? max(sp->dord[o], 0) : 0;
    float4 ca, cb;
    if (OBS && CAPS) {
      ca = reinterpret_cast<const float4*>(obs.spheres)[2 * bi];
      cb = reinterpret_cast<const float4*>(obs.spheres)[2 * bi + 1];
    } else if (OBS) {
      ca = cb = reinterpret_cast<const float4*>(obs.spheres)[bi];
    } else {
      ca = cb = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    size_t off = ((size_t)r0 * P + p) * 3;
    for (int r = 0; r < n_live; ++r, off += (size_t)P * 3) {
      const float4* rec = lds + (size_t)r * W;
      if (is_obs) {
        const float4 sa = rec[2 * leaf];
        f32x3 pl3, po3;
        obstacle_pair_points<LINK, CAPS>(sa, LINK ? rec[2 * leaf + 1] : sa, ca, cb, pl3, po3);
        if (ok) {
          __builtin_nontemporal_store(pl3, reinterpret_cast<f32x3*>(p_link + off));
          __builtin_nontemporal_store(po3, reinterpret_cast<f32x3*>(p_obs + off));
        }
        continue;
      }
      // self pair: leaf o's link against B (an obstacle for the step)
      const float4 la = rec[o_self + 2 * o], lb = rec[o_self + 2 * o + 1];
      const float4 ba = rec[o_b + 2 * bslot], bb = rec[o_b + 2 * bslot + 1];
      const float LA[3] = {la.x, la.y, la.z}, LD[3] = {lb.x - la.x, lb.y - la.y, lb.z - la.z};
      const float laa = dot3(LD, LD);
      const float inv_laa = laa > 0.f ? 1.0f / laa : 0.f;
      float P3[3] = {0.f, 0.f, 0.f};
      float4 rw[3];
      if (point) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rw[c] = rec[o_rot + 3 * o + c], P3[c] = rw[c].w;
      }
      float rr[3], nv[3], dd;
      link_pair_fields(LA, LD, laa, inv_laa, la.w, ba, bb, P3, rr, nv, dd);
      if (!ok) continue;
      if (point) {   // relative_position in the joint frame R^T r, normal_vec, distance (data_management.py:33-53)
        const float rel[3] = {rw[0].x * rr[0] + rw[1].x * rr[1] + rw[2].x * rr[2], rw[0].y * rr[0] + rw[1].y * rr[1] + rw[2].y * rr[2],
                              rw[0].z * rr[0] + rw[1].z * rr[1] + rw[2].z * rr[2]};
        __builtin_nontemporal_store(f32x3{rel[0], rel[1], rel[2]}, reinterpret_cast<f32x3*>(p_link + off));
        __builtin_nontemporal_store(f32x3{nv[0], nv[1], nv[2]}, reinterpret_cast<f32x3*>(p_obs + off));
      } else {       // the two surface points: p_link - p_obs = dd nv
        __builtin_nontemporal_store(f32x3{rr[0], rr[1], rr[2]}, reinterpret_cast<f32x3*>(p_link + off));
        __builtin_nontemporal_store(f32x3{rr[0] - dd * nv[0], rr[1] - dd * nv[1], rr[2] - dd * nv[2]}, reinterpret_cast<f32x3*>(p_obs + off));
      }
      if (dist) __builtin_nontemporal_store(dd, dist + off / 3);
    }
  }
}

// ---- convex-hull link geometry (include/rmp2.h rmp2_set_link_hulls) ---------------------------------------------------------
// The hulls of a handle, compiled by rmp2_set_link_hulls: pair leaf o (ordinal, descriptor order) owns the vertices
// [vert_off[o], vert_off[o + 1]) and the planes [face_off[o], face_off[o + 1]) of the handle's two arrays.
struct HullProg {
  int32_t n_leaves;                           // pair leaves L
  int32_t pad_[3];
  int32_t ord_of_leaf[RMP2_MAX_LEAVES];       // descriptor leaf -> pair-leaf ordinal, -1: not a pair leaf
  int32_t is_point[RMP2_MAX_LEAVES];          // ordinal -> 1: FK_POINT
  int32_t vert_off[RMP2_MAX_LEAVES + 1];
  int32_t face_off[RMP2_MAX_LEAVES + 1];
  // hull self pairs (rmp2_set_self_collision_hulls): S self pairs per robot follow the obstacle pairs in each leaf's range, leaf o's
  // range starting at o K + extra_before[o]; 0 for link hulls (pair leaf o owns [o K, (o + 1) K))
  int32_t n_extra;
  int32_t extra_before[RMP2_MAX_LEAVES];
};

constexpr int kHullRobots = 16;   // robots per wave (as kClosestRobots)

// The write-back of a hull hit of a leaf whose frame is (Rm row-major, t): the leaf's point pl and the other body's point po, both
// in the leaf frame, the unit direction u and the signed gap.  Point leaf: relative_position (frame), normal_vec = sign(g) u
// (base), distance |g|  (link_pair_fields' conventions).  Distance leaf: the two points in the base frame.
// One row layout: rmp2_hull_stage_kernel has its frame as doubles in this form already, rmp2_self_hull_stage_kernel widens its
// [3][4] floats at the call -- the conversions its written-out products made implicitly (registers and scratch are the parent's).
__device__ __forceinline__ void store_hull_pair(const double Rm[9], const double t[3], bool point, double gap, const double u[3],
                                                const double pl[3], const double po[3], float* __restrict__ p_link,
                                                float* __restrict__ p_obs, float* __restrict__ dist, size_t pair) {
  if (point) {
    const double sg = gap >= 0.0 ? 1.0 : -1.0;
    f32x3 nvb;
    nvb.x = (float)(sg * (Rm[0] * u[0] + Rm[1] * u[1] + Rm[2] * u[2]));
    nvb.y = (float)(sg * (Rm[3] * u[0] + Rm[4] * u[1] + Rm[5] * u[2]));
    nvb.z = (float)(sg * (Rm[6] * u[0] + Rm[7] * u[1] + Rm[8] * u[2]));
    __builtin_nontemporal_store(f32x3{(float)pl[0], (float)pl[1], (float)pl[2]}, reinterpret_cast<f32x3*>(p_link + 3 * pair));
    __builtin_nontemporal_store(nvb, reinterpret_cast<f32x3*>(p_obs + 3 * pair));
  } else {
    f32x3 L3, O3;
    L3.x = (float)(Rm[0] * pl[0] + Rm[1] * pl[1] + Rm[2] * pl[2] + t[0]);
    L3.y = (float)(Rm[3] * pl[0] + Rm[4] * pl[1] + Rm[5] * pl[2] + t[1]);
    L3.z = (float)(Rm[6] * pl[0] + Rm[7] * pl[1] + Rm[8] * pl[2] + t[2]);
    O3.x = (float)(Rm[0] * po[0] + Rm[1] * po[1] + Rm[2] * po[2] + t[0]);
    O3.y = (float)(Rm[3] * po[0] + Rm[4] * po[1] + Rm[5] * po[2] + t[1]);
    O3.z = (float)(Rm[6] * po[0] + Rm[7] * po[1] + Rm[8] * po[2] + t[2]);
    __builtin_nontemporal_store(L3, reinterpret_cast<f32x3*>(p_link + 3 * pair));
    __builtin_nontemporal_store(O3, reinterpret_cast<f32x3*>(p_obs + 3 * pair));
  }
  if (dist) __builtin_nontemporal_store((float)fabs(gap), dist + pair);
}

// The hull stage: one wave per kHullRobots robots, as rmp2_closest_wave_kernel.  Phase 1, a lane per robot: a walk of the step's
// program puts each pair leaf's frame (rows of R with the origin in .w) into LDS.  Phase 2, a lane per (robot, record) pair of
// ONE leaf at a time -- the leaf, and with it the hull, is wave-uniform, so its vertices and planes are read through the scalar
// and vector caches at uniform addresses --: the obstacle's axis is brought into the leaf frame (R^T (x - t)), rmp2_hull.h
// hull_closest finds the pair (fp64 GJK, at most kHullGjkIters steps; the face rule where the axis meets the hull), and the
// points go back to the base frame.  Consecutive lanes write consecutive pairs of one robot.
template <int SLOTS, bool CAPS>
__global__ void __launch_bounds__(kWave)
rmp2_hull_stage_kernel(const DevProgram* __restrict__ prog, const HullProg* __restrict__ hp, const float4* __restrict__ hverts,
                       const float4* __restrict__ hplanes, const float* __restrict__ q, const float4* __restrict__ table, int K,
                       float* __restrict__ p_link, float* __restrict__ p_obs, float* __restrict__ dist, int R) {
  extern __shared__ float4 frm[];   // [kHullRobots][L][3]
  const int L = hp->n_leaves;
  const int lane = threadIdx.x;
  const int r0 = blockIdx.x * kHullRobots;
  const int robot = r0 + lane;
  if (lane < kHullRobots && robot < R) {
    const float* my_q = q + (size_t)robot * prog->n_dof;
    // a non-finite q poisons EVERY pair leaf's frame of this robot, those upstream of the joint too (rmp2.h: every pair output
    // of the robot is NaN): a NaN frame makes the axis NaN in phase 2 and hull_closest selects NaN into each field
    const bool qbad = q_is_non_finite(my_q, prog->n_dof);
    const float qn = __builtin_nanf("");
    walk_frames<SLOTS>(prog, my_q, [&](const DevOp& op, const FrameState& cur) {
      for (int li = 0; li < op.leaf_count; ++li) {
        const DevLeaf& lf = prog->leaves[prog->fk_leaves[op.leaf_begin + li]];
        const int o = hp->ord_of_leaf[lf.index];
        if (o < 0) continue;
        float4* rec = frm + ((size_t)lane * L + o) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i)
          rec[i] = make_float4(qbad ? qn : cur.R[3 * i], qbad ? qn : cur.R[3 * i + 1], qbad ? qn : cur.R[3 * i + 2], qbad ? qn : cur.p[i]);
      }
    });
  }
  __syncthreads();
  const int n_live = min(kHullRobots, R - r0);
  const int P = L * K + hp->n_extra;
  for (int o = 0; o < L; ++o) {
    const int v0 = hp->vert_off[o], nv = hp->vert_off[o + 1] - v0;
    const int f0 = hp->face_off[o], nf = hp->face_off[o + 1] - f0;
    const bool point = hp->is_point[o] != 0;
    const int obegin = o * K + hp->extra_before[o];
    for (int it = lane; it < n_live * K; it += kWave) {
      const int r = it / K, k = it - r * K;
      const float4 ca = CAPS ? table[2 * k] : table[k];
      const float4 cb = CAPS ? table[2 * k + 1] : ca;
      const float4* rw = frm + ((size_t)r * L + o) * 3;
      const float4 w0 = rw[0], w1 = rw[1], w2 = rw[2];
      const double Rm[9] = {w0.x, w0.y, w0.z, w1.x, w1.y, w1.z, w2.x, w2.y, w2.z};
      const double t[3] = {w0.w, w1.w, w2.w};
      const double A[3] = {ca.x - t[0], ca.y - t[1], ca.z - t[2]}, B[3] = {cb.x - t[0], cb.y - t[1], cb.z - t[2]};
      double a[3], b[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        a[i] = Rm[i] * A[0] + Rm[3 + i] * A[1] + Rm[6 + i] * A[2];
        b[i] = Rm[i] * B[0] + Rm[3 + i] * B[1] + Rm[6 + i] * B[2];
      }
      // (a capsule record's unused 8th float counts too: non-finite ANYWHERE in a record makes its pairs NaN)
      const double rad = CAPS && !(0.f * cb.w == 0.f) ? (double)__builtin_nanf("") : (double)ca.w;
      const HullHit hh = hull_closest(hverts + v0, nv, hplanes + f0, nf, a, b, rad);
      // the obstacle's surface point c + r u (a distance leaf's p_obs)
      const double po[3] = {hh.xp[0] + rad * hh.u[0], hh.xp[1] + rad * hh.u[1], hh.xp[2] + rad * hh.u[2]};
      store_hull_pair(Rm, t, point, hh.gap, hh.u, hh.hp, po, p_link, p_obs, dist, (size_t)(r0 + r) * P + (size_t)obegin + k);
    }
  }
}

// ---- hull-versus-hull self pairs (include/rmp2.h rmp2_set_self_collision_hulls) -------------------------------------------
// The pair list of a handle with hull self pairs, compiled by rmp2_set_self_collision_hulls.  Hull entry e (frame e, the base
// n_frames) owns the vertices [hv0[e], hv0[e] + hnv[e]) and the planes [hf0[e], hf0[e] + hnf[e]) of the handle's two arrays;
// frame slots are the frames some pair names as A or B (rows of the stage's LDS; the base needs none).
struct SelfHullProg {
  int32_t n_pairs;                           // S = self pairs per robot, grouped by pair-leaf ordinal
  int32_t n_slots;                           // frame slots
  int32_t pad_[2];
  int32_t slot_of_frame[RMP2_MAX_FRAMES];    // frame -> slot, -1: not named by a pair (the marker of the walk)
  int32_t is_point[RMP2_MAX_LEAVES];         // ordinal -> 1: FK_POINT
  int32_t pair_leaf[RMP2_MAX_SELF_PAIRS];    // self pair -> A's pair-leaf ordinal
  int32_t pair_sa[RMP2_MAX_SELF_PAIRS];      // self pair -> A's frame slot
  int32_t pair_sb[RMP2_MAX_SELF_PAIRS];      // self pair -> B's frame slot, -1: the base (identity)
  int32_t pair_ea[RMP2_MAX_SELF_PAIRS];      // self pair -> A's hull entry
  int32_t pair_eb[RMP2_MAX_SELF_PAIRS];      // self pair -> B's hull entry
  int32_t hv0[RMP2_MAX_FRAMES + 1], hnv[RMP2_MAX_FRAMES + 1];
  int32_t hf0[RMP2_MAX_FRAMES + 1], hnf[RMP2_MAX_FRAMES + 1];
};

constexpr int kSelfHullRobots = 64;   // robots per wave: one lane per robot

// visit_frame's pose update without velocities, the parent chosen by selects (identity from the base) rather than by branches:
// the hull self stage's walk needs no scratch this way.  cur = R (row-major) then p.
__device__ __forceinline__ void walk_frame_position(float cur[12], const DevOp& op, float qv, bool from_base) {
  const float ax[3] = {op.axis[0], op.axis[1], op.axis[2]};
  float Rl[9], tl[3];
  if (op.jtype == RMP2_JOINT_REVOLUTE) {
    float sn, cs;
    sincosf(qv, &sn, &cs);
    const float omc = 1.0f - cs;
    const float ut[9] = {0.f, -ax[2], ax[1], ax[2], 0.f, -ax[0], -ax[1], ax[0], 0.f};
    float Rv[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) Rv[3 * r + k] = cs * (r == k ? 1.f : 0.f) + sn * ut[3 * r + k] + omc * (ax[r] * ax[k]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) Rl[3 * r + k] = op.Tc[4 * r + 0] * Rv[k] + op.Tc[4 * r + 1] * Rv[3 + k] + op.Tc[4 * r + 2] * Rv[6 + k];
#pragma unroll
    for (int r = 0; r < 3; ++r) tl[r] = op.Tc[4 * r + 3];
  } else {
    const float qp = op.jtype == RMP2_JOINT_PRISMATIC ? qv : 0.f;
    const float tv[3] = {qp * ax[0], qp * ax[1], qp * ax[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) Rl[3 * r + k] = op.Tc[4 * r + k];
      tl[r] = op.Tc[4 * r + 0] * tv[0] + op.Tc[4 * r + 1] * tv[1] + op.Tc[4 * r + 2] * tv[2] + op.Tc[4 * r + 3];
    }
  }
  float Rp[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) Rp[c] = from_base ? ((c == 0 || c == 4 || c == 8) ? 1.f : 0.f) : cur[c];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) cur[3 * i + k] = Rp[3 * i + 0] * Rl[k] + Rp[3 * i + 1] * Rl[3 + k] + Rp[3 * i + 2] * Rl[6 + k];
    cur[9 + i] = Rp[3 * i + 0] * tl[0] + Rp[3 * i + 1] * tl[1] + Rp[3 * i + 2] * tl[2] + Rp[9 + i];
  }
}

// The hull self-pair stage.  One wave per nr (64 unless the frame slots overflow 64 KiB of LDS) robots, a lane per robot in both
// phases.  Phase 1: a walk of the unpruned program (`prog_full`) puts the frame of every slot into LDS, [slot][12][nr] floats
// (rows of R with the origin in the 4th column), so each lane reads its own robot's frames without bank conflicts.  The walk is
// its own, not walk_frames: restore and save are selects over every slot (and walk_frame_position picks the parent by selects),
// so no array is indexed at run time and the kernel needs no scratch.  Phase 2: the
// self pairs one after another -- the pair, and with it both hulls, is wave-uniform, so their vertices and planes are read at
// uniform addresses through the scalar cache and the support loops have a uniform trip count --: B is placed in A's frame
// (R_A^T R_B, R_A^T (p_B - p_A)) and rmp2_hull.h hull_pair_closest finds the pair (fp64 GJK, at most kPairGjkIters steps; the face
// rule where the hulls overlap).  Self pair j of leaf o goes to entry (o + 1) K + j of the robot's P pairs: each leaf's range is
// [K obstacle pairs | S_l self pairs] (K = 0 without a table; with one, every pair leaf is a distance leaf).
template <int SLOTS>
__global__ void __launch_bounds__(kWave)
rmp2_self_hull_stage_kernel(const DevProgram* __restrict__ prog_full, const SelfHullProg* __restrict__ sp, const float4* __restrict__ hverts,
                            const float4* __restrict__ hplanes, const float* __restrict__ q, float* __restrict__ p_link,
                            float* __restrict__ p_obs, float* __restrict__ dist, int P, int K, int R, int nr) {
  extern __shared__ float frs[];   // [n_slots][12][nr]
  const int lane = threadIdx.x;
  const int robot = blockIdx.x * nr + lane;
  if (lane >= nr || robot >= R) return;   // (no barrier below: a lane reads only what it wrote)
  bool qbad;   // a non-finite q: every pair of this robot is NaN, whichever frames it names (rmp2.h)
  {
    const float* my_q = q + (size_t)robot * prog_full->n_dof;
    qbad = q_is_non_finite(my_q, prog_full->n_dof);
    float cur[12];   // R row-major, then p  (visit_frame's positions; no velocities)
    float saved[SLOTS > 0 ? SLOTS : 1][12];
#pragma unroll
    for (int c = 0; c < 12; ++c) cur[c] = 0.f;
    for (int k = 0; k < prog_full->n_ops; ++k) {
      const DevOp& op = prog_full->ops[k];
      if (SLOTS > 0 && op.restore >= 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
#pragma unroll
          for (int c = 0; c < 12; ++c) cur[c] = op.restore == s ? saved[s][c] : cur[c];
      }
      walk_frame_position(cur, op, op.qidx >= 0 ? my_q[op.qidx] : 0.f, op.restore == -2);
      if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
#pragma unroll
          for (int c = 0; c < 12; ++c) saved[s][c] = op.save == s ? cur[c] : saved[s][c];
      }
      const int fs = sp->slot_of_frame[op.frame];
      if (fs < 0) continue;
      float* rec = frs + (size_t)fs * 12 * nr + lane;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rec[(4 * i + c) * nr] = cur[3 * i + c];
        rec[(4 * i + 3) * nr] = cur[9 + i];
      }
    }
  }
  const size_t row = (size_t)robot * P;
  for (int j = 0; j < sp->n_pairs; ++j) {
    const int o = sp->pair_leaf[j], sa = sp->pair_sa[j], sb = sp->pair_sb[j], ea = sp->pair_ea[j], eb = sp->pair_eb[j];
    float A[12], B[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) A[c] = frs[((size_t)sa * 12 + c) * nr + lane];
    if (sb >= 0) {
#pragma unroll
      for (int c = 0; c < 12; ++c) B[c] = frs[((size_t)sb * 12 + c) * nr + lane];
    } else {   // the fixed base
#pragma unroll
      for (int c = 0; c < 12; ++c) B[c] = (c == 0 || c == 5 || c == 10) ? 1.f : 0.f;
    }
    // B in A's frame: Rm = R_A^T R_B, t = R_A^T (p_B - p_A)   (R_X[i][c] = X[4 i + c], p_X[i] = X[4 i + 3])
    double Rm[9], t[3];
    const double dp[3] = {(double)B[3] - (double)A[3], (double)B[7] - (double)A[7], (double)B[11] - (double)A[11]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        Rm[3 * i + c] = (double)A[i] * (double)B[c] + (double)A[4 + i] * (double)B[4 + c] + (double)A[8 + i] * (double)B[8 + c];
      const double ti = (double)A[i] * dp[0] + (double)A[4 + i] * dp[1] + (double)A[8 + i] * dp[2];
      t[i] = qbad ? (double)__builtin_nanf("") : ti;   // hull_pair_closest selects NaN into every field
    }
    const PairHit hh = hull_pair_closest(hverts + sp->hv0[ea], sp->hnv[ea], hplanes + sp->hf0[ea], sp->hnf[ea], hverts + sp->hv0[eb],
                                         sp->hnv[eb], hplanes + sp->hf0[eb], sp->hnf[eb], Rm, t);
    // A's frame (p_link = R_A pa + p_A, p_obs = R_A pb + p_A for a distance leaf)
    const double Ra[9] = {A[0], A[1], A[2], A[4], A[5], A[6], A[8], A[9], A[10]}, ta[3] = {A[3], A[7], A[11]};
    store_hull_pair(Ra, ta, sp->is_point[o] != 0, hh.gap, hh.u, hh.pa, hh.pb, p_link, p_obs, dist, row + (size_t)K * (o + 1) + j);
  }
}

// x = vec(T_frame), xd = J qd, J = d vec(T)/dq, c = Jdot qd   (kinematics.py:250-270)
template <int SLOTS>
__global__ void __launch_bounds__(kWave)
rmp2_diff_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ q, const float* __restrict__ qd,
                 int frame, float* __restrict__ xo, float* __restrict__ xdo, float* __restrict__ Jo,
                 float* __restrict__ co, float* __restrict__ zo_scratch, int R, int euler) {
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  const int n = prog->n_dof;
  const float* my_q = q + (size_t)robot * n;
  const float* my_qd = qd + (size_t)robot * n;
  float* zo = zo_scratch + (size_t)robot * 6 * RMP2_MAX_DOF;  // per-robot z_j, o_j (global scratch)
  FrameState cur;
  FrameState slot[SLOTS > 0 ? SLOTS : 1];
  for (int k = 0; k < prog->n_ops; ++k) {
    const DevOp& op = prog->ops[k];
    if (SLOTS > 0 && op.restore >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.restore == s) cur = slot[s];
    }
    const int qi = op.qidx;
    float z[3];
    visit_frame<true>(cur, op, qi >= 0 ? my_q[qi] : 0.f, qi >= 0 ? my_qd[qi] : 0.f, op.restore == -2, z);
    if (qi >= 0 && op.jtype != RMP2_JOINT_FIXED) {
      for (int c = 0; c < 3; ++c) {
        zo[qi * 6 + c] = z[c];
        zo[qi * 6 + 3 + c] = cur.p[c];
      }
    }
    if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.save == s) slot[s] = cur;
    }
    if (op.frame != frame) continue;
    if (euler) {
      // chain [FK(frame), 4x4 -> Euler xyz] (taskmap.py:57-67, kinematics.py:74-96): R = Rz Ry Rx, angular velocity
      // w = H(e) ed with H = [Rz Ry ex | Rz ey | ez]; J = H^-1 J_w (J_w: world axes of the revolute ancestors)
      const float r00 = cur.R[0], r10 = cur.R[3], r20 = cur.R[6], r21 = cur.R[7], r22 = cur.R[8];
      const float ty = -asinf(r20);
      const float cy = cosf(ty), sy = -r20;
      const float safe = fabsf(cy) < 1e-6f ? 1.0f : cy;  // the reference's guard on the VALUE (kinematics.py:88)
      const float tz = atan2f(r10 / safe, r00 / safe), tx = atan2f(r21 / safe, r22 / safe);
      const float cz = cosf(tz), sz = sinf(tz);
      auto hinv = [&](const float u[3], float o[3]) {
        const float a = (cz * u[0] + sz * u[1]) / cy;
        o[0] = a;
        o[1] = -sz * u[0] + cz * u[1];
        o[2] = u[2] + sy * a;
      };
      float* x = xo + (size_t)robot * 3;
      float* xd = xdo + (size_t)robot * 3;
      float* c = co + (size_t)robot * 3;
      float* J = Jo + (size_t)robot * 3 * n;
      x[0] = tx, x[1] = ty, x[2] = tz;
      float ed[3];
      hinv(cur.w, ed);
      for (int i = 0; i < 3; ++i) xd[i] = ed[i];
      for (int j = 0; j < n; ++j) {
        float col[3] = {0.f, 0.f, 0.f};
        if (((op.anc_mask >> j) & 1u) && ((prog->rev_mask >> j) & 1u)) {
          const float zj[3] = {zo[j * 6], zo[j * 6 + 1], zo[j * 6 + 2]};
          hinv(zj, col);
        }
        for (int i = 0; i < 3; ++i) J[i * n + j] = col[i];
      }
      // Hdot ed: d/dt of the columns (cz cy, sz cy, -sy) and (-sz, cz, 0)
      const float h0[3] = {-sz * cy * ed[2] - cz * sy * ed[1], cz * cy * ed[2] - sz * sy * ed[1], -cy * ed[1]};
      const float h1[3] = {-cz * ed[2], -sz * ed[2], 0.f};
      const float rhs[3] = {cur.al[0] - (h0[0] * ed[0] + h1[0] * ed[1]), cur.al[1] - (h0[1] * ed[0] + h1[1] * ed[1]),
                            cur.al[2] - (h0[2] * ed[0] + h1[2] * ed[1])};
      float cc[3];
      hinv(rhs, cc);
      for (int i = 0; i < 3; ++i) c[i] = cc[i];
      return;
    }
    float* x = xo + (size_t)robot * 16;
    float* xd = xdo + (size_t)robot * 16;
    float* c = co + (size_t)robot * 16;
    float* J = Jo + (size_t)robot * 16 * n;
    for (int i = 0; i < 16 * n; ++i) J[i] = 0.f;
    for (int i = 0; i < 16; ++i) x[i] = xd[i] = c[i] = 0.f;
    x[15] = 1.f;
    for (int col = 0; col < 3; ++col) {
      const float Rc[3] = {cur.R[col], cur.R[3 + col], cur.R[6 + col]};
      float wxR[3], alxR[3], wwR[3];
      cross3(cur.w, Rc, wxR);
      cross3(cur.al, Rc, alxR);
      cross3(cur.w, wxR, wwR);
      for (int row = 0; row < 3; ++row) {
        x[4 * row + col] = Rc[row];
        xd[4 * row + col] = wxR[row];
        c[4 * row + col] = alxR[row] + wwR[row];
      }
      for (int j = 0; j < n; ++j) {
        if (!((op.anc_mask >> j) & 1u) || !((prog->rev_mask >> j) & 1u)) continue;
        const float zj[3] = {zo[j * 6], zo[j * 6 + 1], zo[j * 6 + 2]};
        float zxR[3];
        cross3(zj, Rc, zxR);
        for (int row = 0; row < 3; ++row) J[(4 * row + col) * n + j] = zxR[row];
      }
    }
    for (int j = 0; j < n; ++j) {
      if (!((op.anc_mask >> j) & 1u)) continue;
      const float zj[3] = {zo[j * 6], zo[j * 6 + 1], zo[j * 6 + 2]};
      float cj[3] = {zj[0], zj[1], zj[2]};
      if ((prog->rev_mask >> j) & 1u) {
        const float d[3] = {cur.p[0] - zo[j * 6 + 3], cur.p[1] - zo[j * 6 + 4], cur.p[2] - zo[j * 6 + 5]};
        cross3(zj, d, cj);
        if ((op.anc_mask >> (16 + j)) & 1u) cj[0] = cj[1] = cj[2] = 0.f;   // the origin lies on joint j's axis (structural_lever_zeros)
      }
      for (int row = 0; row < 3; ++row) J[(4 * row + 3) * n + j] = cj[row];
    }
    for (int row = 0; row < 3; ++row) {
      x[4 * row + 3] = cur.p[row];
      xd[4 * row + 3] = cur.v[row];
      c[4 * row + 3] = cur.a[row];
    }
    return;
  }
}

}  // namespace

/*
 * rmp2.h -- C ABI of the MI355X RMP2 evaluation-and-pullback engine (librmp2_hip.so).
 *
 * The reference (TomGoesGitHub/Riemannian-Motion-Policies) has no FFI: its seam is the
 * Python protocol  RmpCore.evaluate(q, qd) -> qdd  (rmp.py:133-155).  This header is the
 * C boundary that replaces everything below that call -- task-map differentiation
 * (taskmap.py:13-168, kinematics.py:212-270, helper/rmp_helper.py:3-60), leaf evaluation
 * (rmp2.py:31-226, rmp.py:226-382), the pull-back and sum (rmp.py:157-180, :142-150) and the
 * resolve step (rmp.py:153-154) -- for a BATCH of R independent robots of one type.
 *
 * Rules of the boundary
 *   - plain C, plain pointers and sizes; no C++/torch types.
 *   - the caller owns every buffer; the engine owns its handle, its constant tables and
 *     nothing else.  rmp2_step() allocates nothing and never synchronises the host -- one exception: a handle
 *     whose every robot is resolved by the pseudo-inverse (solve_mode = PINV, or a set without a positive-definite
 *     identity-map leaf) on a 3..9-dof robot keeps the combined systems of the fleet between its two kernels
 *     (8 n (n + 1) bytes per robot) and grows that buffer, synchronising, the first time a larger fleet is stepped.
 *   - all array arguments of rmp2_step / rmp2_forward_kinematics / rmp2_differentiate are
 *     DEVICE pointers (HBM), row-major, robot index slowest: q[R][n_dof] etc.
 *   - every call returns 0 on success or a negative RMP2_ERR_* code; the message is
 *     available from rmp2_last_error().
 *   - a handle is bound to one device; calls on one handle must not race (thread-compatible).
 *     rmp2_create and the launching calls make that device the calling thread's current HIP device
 *     (as hipSetDevice would) and leave it so; rmp2_destroy restores the caller's.
 *   - there is NO host/CPU execution path in this library.  If no HIP device is usable,
 *     rmp2_create() fails with RMP2_ERR_NO_DEVICE.
 */
#ifndef RMP2_H
#define RMP2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMP2_ABI_VERSION 5 /* 5: self collision (rmp2_set_self_collision, rmp2_self_pairs); 4: rmp2_reserve, rmp2_exchange_nranks,
                              RMP2_STATUS_JACOBI; attached-point leaves take a table + link_capsules */

#define RMP2_MAX_FRAMES 32  /* frames (= URDF joints) per robot type                    */
#define RMP2_MAX_DOF 16     /* actuated joints per robot type                            */
#define RMP2_MAX_LEAVES 48  /* leaf RMPs per set                                          */
#define RMP2_MAX_PARAMS 12  /* scalar parameters per leaf                                 */
#define RMP2_MAX_SELF_PAIRS 256 /* self-collision pairs per robot (rmp2_set_self_collision) */
#define RMP2_MAX_HULL_VERTICES 512 /* vertices per link hull (rmp2_set_link_hulls)          */
#define RMP2_MAX_HULL_FACES 1024   /* face planes per link hull (rmp2_set_link_hulls)       */

/* ---- error codes --------------------------------------------------------------------- */
#define RMP2_OK 0
#define RMP2_ERR_INVALID_ARGUMENT (-1)
#define RMP2_ERR_UNSUPPORTED (-2) /* no kernel for this combination (e.g. > 2 open branch points; solve = PINV,
                                     sets without an inertia leaf or attached-point leaves beyond 9 dofs) */
#define RMP2_ERR_NO_DEVICE (-3)
#define RMP2_ERR_HIP (-4)         /* a HIP runtime call failed; see rmp2_last_error()      */
#define RMP2_ERR_ABI_MISMATCH (-5)

/* ---- robot table (output of the URDF "kinematic compiler") ---------------------------
 * Replaces the tensors built by UrdfForwardKinematic._build (kinematics.py:163-209):
 * kinematic_chains -> parent[], _q_reordering -> q_index[], T_constant, axis,
 * is_revolute/is_prismatic/is_fixed -> joint_type[].  Frame order = reference frame order
 * (breadth-first, helper/urdf_parsing.py:74-97). */
#define RMP2_JOINT_FIXED 0
#define RMP2_JOINT_REVOLUTE 1
#define RMP2_JOINT_PRISMATIC 2

typedef struct rmp2_robot {
  int32_t n_frames;
  int32_t n_dof;
  int32_t parent[RMP2_MAX_FRAMES];     /* parent frame, -1 = attached to the base link      */
  int32_t joint_type[RMP2_MAX_FRAMES]; /* RMP2_JOINT_*                                      */
  int32_t q_index[RMP2_MAX_FRAMES];    /* index into q, -1 = evaluated at q = 0             */
  float axis[RMP2_MAX_FRAMES][3];      /* joint axis in the joint frame                     */
  float T_const[RMP2_MAX_FRAMES][12];  /* rows 0..2 of the 4x4 T_constant, row-major        */
} rmp2_robot;

/* ---- leaf policies -------------------------------------------------------------------
 * kind: which (xdd_des, A) formula; each cites the reference class it reproduces,
 * quirks included.  params[] order is the reference
 * constructor's keyword order. */
#define RMP2_LEAF_TARGET_ATTRACTOR 1 /* rmp2.py:31-83   params: accel_p_gain, accel_d_gain, accel_norm_eps,
                                        metric_alpha_length_scale, min_metric_alpha, max_metric_scalar,
                                        min_metric_scalar, proximity_metric_boost_scalar,
                                        proximity_metric_boost_length_scale ; goal: 3 floats   */
#define RMP2_LEAF_JOINT_VELOCITY_CAP 2 /* rmp2.py:86-112  params: max_velocity, velocity_damping_region,
                                        damping_gain, metric_weight                          */
#define RMP2_LEAF_JOINT_DAMPING 3    /* rmp2.py:115-137 params: accel_d_gain, metric_scalar, inertia */
#define RMP2_LEAF_OBSTACLE_AVOIDANCE 4 /* rmp2.py:140-196 params: margin, damping_gain, damping_std_dev,
                                        damping_robustness_eps, damping_velocity_gate_length_scale,
                                        repulsion_gain, repulsion_std_dev, metric_modulation_radius,
                                        metric_scalar, metric_exploder_std_dev, metric_exploder_eps */
#define RMP2_LEAF_CSPACE_BIASING 5   /* rmp2.py:198-226 params: metric_scalar, position_gain, damping_gain,
                                        robust_position_term_thresh, inertia ; vec_a = goal q0 */
#define RMP2_LEAF_TARGET_POLICY 6    /* rmp.py:226-260  params: alpha, beta, c ; goal: k floats
                                        (k = 3 on an FK position map, n_dof on the identity map) */
#define RMP2_LEAF_JOINT_LIMIT_AVOIDANCE 7 /* rmp.py:349-382 params: gamma_p, gamma_d ;
                                        vec_a = lower limits, vec_b = upper limits             */
#define RMP2_LEAF_CONFIG_SPACE_BIASING 8 /* rmp.py:318-347 params: gamma_p, gamma_d, w ; vec_a = q0 */
#define RMP2_LEAF_COLLISION_AVOIDANCE 9 /* rmp.py:264-315 params: eta_rep, nu_rep, eta_damp, nu_damp, r, c ;
                                        per-pair data d, n (rmp2_obstacles.dist / p_obs), FK_POINT map only.
                                        beta = 0 in the reference (rmp.py:311) => metric w(d) * I          */

/* task map of a leaf (the chains the reference's experiments build with chain_taskmaps,
 * taskmap.py:142-168) */
#define RMP2_TASKMAP_IDENTITY 0    /* IdentityTaskmap                  taskmap.py:13-20        */
#define RMP2_TASKMAP_FK_POSITION 1 /* FK(frame) -> 4x4 -> position     taskmap.py:22-31,45-54  */
#define RMP2_TASKMAP_FK_DISTANCE 2 /* FK(frame) -> 4x4 -> distance     taskmap.py:22-31,115-138 */
#define RMP2_TASKMAP_FK_POINT 3    /* FK(frame) -> relative 4x4 -> position   taskmap.py:22-31,79-99,45-54:
                                      a point rigidly attached to the frame, one per pair (position given in the
                                      JOINT frame, rmp2_obstacles.p_link); lever arm included, unlike FK_DISTANCE */

typedef struct rmp2_leaf {
  int32_t kind;        /* RMP2_LEAF_*                                                     */
  int32_t taskmap;     /* RMP2_TASKMAP_*                                                  */
  int32_t frame;       /* frame index for FK task maps, else -1                           */
  int32_t goal_offset; /* float offset of this leaf's goal inside one robot's goal row, -1 = none */
  float params[RMP2_MAX_PARAMS];
  float vec_a[RMP2_MAX_DOF];
  float vec_b[RMP2_MAX_DOF];
} rmp2_leaf;

/* ---- resolve step ------------------------------------------------------------------ */
#define RMP2_SOLVE_AUTO 0 /* fp64 LU with threshold pivoting; robots whose metric is (numerically)
                             singular fall through to the PINV path.  Same result as PINV to fp64
                             rounding whenever M is well conditioned.                         */
#define RMP2_SOLVE_PINV 1 /* reference-faithful: qdd = pinv(M) f, the fp64 Moore-Penrose pseudo-inverse with
                             TensorFlow's cutoff 10*n*eps*sigma_max (rmp.py:153).  Where the elimination can CERTIFY
                             that every singular value of a robot's M lies above the cutoff (sets with an inertia
                             leaf: a bound on |M^-1| from its own triangular factor), pinv(M) = inv(M) and the
                             elimination's result stands; every other robot -- and every robot of a set without
                             an inertia leaf -- is resolved by a one-sided Jacobi SVD (status RMP2_STATUS_JACOBI /
                             RANK_DROP).  Same numbers either way to fp64 rounding; the certifying step costs
                             what the AUTO step costs.                                                      */

typedef struct rmp2_desc {
  int32_t abi_version; /* must be RMP2_ABI_VERSION */
  int32_t solve_mode;  /* RMP2_SOLVE_* */
  int32_t n_leaves;
  int32_t goal_floats; /* floats per robot in the goal array (sum over goal-bearing leaves) */
  rmp2_robot robot;
  rmp2_leaf leaves[RMP2_MAX_LEAVES];
} rmp2_desc;

/* ---- per-step obstacle input (data of the distance task maps) -----------------------
 * The reference feeds closest-point pairs through Datamanager tf.Variables
 * (data_management.py:8-17, taskmap.py:115-138).  Two array-backed forms:
 *   EXPLICIT_PAIRS (reference-faithful): for every FK_DISTANCE leaf l a block of pairs
 *     p_link[r][pair_begin[l] .. pair_begin[l+1])[3], p_obs[...] in the robot base frame.
 *     value d = |p_link - p_obs|; derivative w.r.t. the FRAME ORIGIN only (quirk Q5).
 *     For an FK_POINT leaf (CollisionAvoidance) the same pair range carries the Datamanager's
 *     other three fields (data_management.py:14-16): p_link = 'relative_position' in the joint
 *     frame, p_obs = 'normal_vec' in the base frame, dist[r][pair] = 'distance'.
 *   SHARED_SPHERES: one table spheres[K][4] = (cx, cy, cz, radius) for the whole fleet;
 *     every FK_DISTANCE leaf sees K pairs: control point = its frame origin,
 *     d = |origin - c| - radius, direction (origin - c)/|origin - c|.
 *   RAGGED_SPHERES: as SHARED_SPHERES but robot r only sees the spheres
 *     csr_index[csr_offset[r] .. csr_offset[r+1]) .
 * Both table modes take either primitive:
 *   PRIM_SPHERE  record = 4 floats (cx, cy, cz, radius)
 *   PRIM_CAPSULE record = 8 floats (ax, ay, az, radius, bx, by, bz, unused): a segment a-b swept by a
 *     sphere (the reference's cylinder obstacles, simulation.py:245-261, :495-500).  The engine forms the
 *     closest point of the segment to the control point, c* = a + clamp((p-a).(b-a)/|b-a|^2, 0, 1)(b-a),
 *     and proceeds as for a sphere centred at c*: this IS the closest-point preprocessing the reference
 *     runs on the CPU before every step (simulation.py:462-484 calculate_distances -> Datamanager),
 *     fused into the step.  rmp2_closest_points() below materialises the same pairs as arrays.
 */
#define RMP2_OBS_NONE 0
#define RMP2_OBS_EXPLICIT_PAIRS 1
#define RMP2_OBS_SHARED_SPHERES 2
#define RMP2_OBS_RAGGED_SPHERES 3

#define RMP2_PRIM_SPHERE 0
#define RMP2_PRIM_CAPSULE 1
#define RMP2_PRIM_CYLINDER 2 /* record = 8 floats (cx, cy, cz, radius, ux, uy, uz, half_height): a finite cylinder with FLAT caps, centre c, unit
                              * axis u -- the reference's own obstacle primitive (simulation.py:245-261: pybullet.GEOM_CYLINDER).  Table modes:
                              * x = signed distance of the control point to the cylinder's surface, direction = its outward normal there
                              * (side, cap or rim).  rmp2_closest_points[_links]: the nearest points of the link (its capsule, or the frame
                              * origin) and the cylinder's surface.  Not with link_capsules fused into the step (that closed form is an
                              * iteration: run the stage and feed EXPLICIT_PAIRS). */

typedef struct rmp2_obstacles {
  int32_t mode;
  int32_t n_spheres;                       /* K = records in the primitive table             */
  int32_t n_pairs;                         /* P = pairs per robot, EXPLICIT_PAIRS            */
  int32_t primitive;                       /* RMP2_PRIM_* (table modes)                      */
  int32_t pair_begin[RMP2_MAX_LEAVES + 1]; /* indexed by LEAF index; non-distance leaves: empty range */
  const float *spheres;                    /* device [K][4] spheres or [K][8] capsules       */
  const float *p_link;                     /* device [R][P][3]                               */
  const float *p_obs;                      /* device [R][P][3]                               */
  const int32_t *csr_offset;               /* device [R+1]                                   */
  const int32_t *csr_index;                /* device [csr_offset[R]]; non-null even when every list is empty */
  const float *dist;                       /* device [R][P], FK_POINT leaves only (else NULL) */
  const float *link_capsules;              /* device [n_distance_leaves][8] = (a, radius, b, -) in each distance leaf's FRAME
                                              coordinates (leaf order), or NULL.  Table modes: the control point of a pair is
                                              the nearest point of the LINK's capsule to the obstacle -- the values of
                                              rmp2_closest_points_links + EXPLICIT_PAIRS (d = |p_link - p_obs| and unit normal; as
                                              there, the derivative moves the point with the frame origin, taskmap.py:124-129).
                                              Where the two axes INTERSECT (a sphere centred on the link's axis, crossing segments)
                                              there is no common normal: every route takes the fixed direction +z, so the shapes
                                              overlap by the sum of their radii along it and the pair's normal is -z.
                                              FUSED into the step for tables of at most 256 spheres / capsules, robots with at
                                              most 9 dofs and an inertia leaf, solve = AUTO or a certifying PINV, and 2-dof robots
                                              with either resolve (their closed-form 2 x 2 resolve is the pseudo-inverse) -- shared
                                              tables, ragged lists, rollouts; a plain step beyond those limits -- more dofs, the
                                              all-Jacobi PINV, bigger tables, CYLINDER tables -- runs as the stage into the
                                              handle's stage buffer followed by the explicit-pair step (two launches, same numbers as
                                              calling the two entry points).  RAGGED lists take that route with one more launch (one
                                              pair per list entry, a repeated index counted twice as in the fused form, filler pairs
                                              1e9 m away up to the fleet's longest list); the list lengths are read back from
                                              csr_offset, so that form synchronises the stream and is refused inside a stream capture.
                                              The stage buffer holds 24 n_dist K (+ 24 n_dist L over ragged lists) bytes per robot,
                                              grown on demand like the other staged routes' (see rmp2_set_self_collision): refused
                                              with RMP2_ERR_UNSUPPORTED and the byte count beyond the free device memory, and inside a
                                              stream capture.
                                              Rollouts beyond the fused limits, and sets with attached-point leaves over ragged
                                              lists: RMP2_ERR_UNSUPPORTED. */
} rmp2_obstacles;

/* ---- outputs ----------------------------------------------------------------------- */
#define RMP2_STATUS_NONFINITE 1u /* qdd contains NaN/Inf.  A FINITE state reaches two poles of the reference: JointVelocityCap's (quirk
                                  * Q4: a joint with |qd| == (max_velocity - velocity_damping_region) - velocity_damping_region in
                                  * fp32, where the metric is w / (1 - 1)), and a distance leaf's control point ON its obstacle's
                                  * surface or centre (the curvature term of the distance map divides by the surface distance, the
                                  * normal by the distance to the centre).  Such a robot's SYSTEM is non-finite, and it resolves to
                                  * NaN on EVERY joint with this bit, in every mapping and both resolves
                                  * (tests/test_gpu_leaf_edges.py).  A robot fed a NaN / Inf in q or qd
                                  * resolves to NaN on EVERY joint with this bit: the non-finite dof's force is made non-finite by
                                  * construction, so that neither the culling (an out-of-range pair -- metric 0, acceleration NaN in
                                  * the reference: 0 * NaN -- is never evaluated here) nor a set that never reads the joint can return
                                  * a finite answer for it.  This is the reference's result wherever its own arithmetic carries the
                                  * value into the system (tf.linalg.pinv of a non-finite system is NaN), and stricter where it does
                                  * not (a joint that moves no leaf frame in a set without identity-map leaves). */
#define RMP2_STATUS_RANK_DROP 2u /* the pseudo-inverse dropped at least one singular value  */
#define RMP2_STATUS_PINV_PATH 4u /* AUTO mode: this robot was resolved on the PINV path      */
#define RMP2_STATUS_JACOBI 8u    /* PINV mode, certifying step (symmetric sets with an inertia leaf): the elimination could not
                                  * certify this robot's metric as full rank above TensorFlow's cutoff, so it was resolved by the
                                  * Jacobi pseudo-inverse instead of by the elimination (same result where both apply; diagnostic) */

typedef struct rmp2_outputs {
  float *qdd;       /* device [R][n_dof]                      required                     */
  uint32_t *status; /* device [R]                             optional (NULL)              */
  double *M;        /* device [R][n_dof][n_dof] combined metric,   optional (NULL)         */
  double *f;        /* device [R][n_dof]        combined force,    optional (NULL)         */
} rmp2_outputs;

typedef struct rmp2_handle rmp2_handle;

/* Library/ABI identification (bindings check these before anything else). */
int rmp2_abi_version(void);
size_t rmp2_sizeof_desc(void);
size_t rmp2_sizeof_obstacles(void);

/* The reference's LEAF protocol on its own:  rmp.evaluate(x, xd) -> (xdd_des, A)  (rmp2.py:25-29, rmp.py:202-206) for a
 * batch of B task-space points, outside any RmpCore (rmp2_step evaluates the leaves inside the fused control step and
 * never calls this).  `leaf`: kind + params (+ vec_a / vec_b) as in rmp2_desc; taskmap / frame / goal_offset ignored.
 *   k           task-space dimension: 3 (TargetAttractor, CollisionAvoidance), 1 (ObstacleAvoidance), 1 .. RMP2_MAX_DOF
 *               for the identity-map leaves and TargetPolicy
 *   x, xd       device [B][k];   goal  device [k] (TargetAttractor, TargetPolicy) else NULL
 *   dist, nvec  device [B], [B][3]: CollisionAvoidance's data-fed distance / normal (else NULL)
 *   xdd, A      device [B][k], [B][k][k] (row major)
 * TargetPolicy's norms are global in the reference (rmp.py:243: B = 1 there); here every row is its own evaluation. */
int rmp2_leaf_evaluate(int device, const rmp2_leaf *leaf, int32_t k, const float *x, const float *xd, const float *goal,
                       const float *dist, const float *nvec, float *xdd, float *A, int32_t B, void *stream);

/* Dry run of rmp2_create's host-side program compiler (descriptor validation, depth-first schedule with save / restore
 * slots, pruning and folding of leaf-less fixed frames, ancestor / dof tables): RMP2_OK or the error rmp2_create would
 * return for this descriptor, message via rmp2_last_error(NULL).  Needs no HIP device -- it is what a host-side tool
 * (and the sanitizer build, tools/asan_compile_program.sh) can exercise without a GPU. */
int rmp2_validate(const rmp2_desc *desc);

/* Host-side view of what the program compiler prepares for the quad mapping's structured identity-leaf loop: when EVERY
 * identity-map leaf of the set is JointDamping, CSpaceBiasing, configuration-space biasing or JointVelocityCap, one 32-word
 * record per such leaf, in execution order, is written to `records` (at most `capacity` of them) --
 *   word 0 kind (int32) | 1 P[0] - P[1] | 2 P[1] - 1e-6f | 3 P[0] + P[4] (fp32, rounded once) | 4..15 P[0..11] | 16..31 vec_a[0..15]
 * -- and their number is returned; 0 when the set has no identity leaf or a dense one (JointLimitAvoidance, TargetPolicy on
 * the identity map: such a set keeps the general loop), a negative RMP2_ERR_* code as rmp2_validate.  Needs no HIP device. */
int rmp2_identity_records(const rmp2_desc *desc, void *records, int32_t capacity);

/* Environment variables read by rmp2_create (and by nothing else).  They are DIAGNOSTIC overrides of the per-call kernel
 * dispatch, used by the parity tests and the profiling tools to force every mapping over the same inputs; all choices
 * produce the same numbers to fp32 rounding, none is needed for correctness, and an unset variable means "by fleet size":
 *   RMP2_KERNEL     = hex | quad | lane   mapping of robots to lanes (16 / 4 / 1 lanes per robot);
 *                                         lane also selects the lane-per-robot form of the closest-point stage
 *   RMP2_QUAD_MINW  = 2 | 3 | 4           register cap of the quad mapping's throughput build (waves per SIMD it leaves room for)
 *   RMP2_QUAD_SYM   = 0                   general (full-matrix) form of the quad mapping for sets that qualify for the symmetric one
 *   RMP2_EXCHANGE_THROTTLE_US = n         (rmp2_exchange_create) bound of the host throttle of rmp2_exchange_step, 0 = free-running
 *   RMP2_EXCHANGE_BUFFERS = 2 | 3         (rmp2_exchange_create) table buffers in rotation: 3 (default), or depth + 1
 *   RMP2_EXPLICIT_GLDS = 1                (rmp2_create) EXPLICIT_PAIRS: the pair arrays streamed half a leaf ahead by LDS-DMA with per-quad
 *                                         compaction of the in-range pairs (built and parity-tested in round 4; measured no faster than
 *                                         the register loads -- the mode is bound by the bytes a CU can keep in flight beside the frame
 *                                         records in LDS --, so it is off by default)
 *   RMP2_EXPLICIT_STREAM = 1              (rmp2_create) EXPLICIT_PAIRS, plain control step: the streamed form (pair phase of all leaf
 *                                         frames before the pull-back, pair arrays by LDS-DMA through the frame records' LDS, four
 *                                         waves per SIMD) -- built, parity-tested and measured in round 5: not faster while the whole
 *                                         fleet is one round of waves, so it is off by default
 *   RMP2_STREAM_STAGGER = n               (rmp2_create) with it: start offset between the four waves of a SIMD (units of 3.4 us; A/B)
 *   RMP2_STRICT_CERTIFY = 0               (rmp2_create) solve = PINV: the Jacobi pseudo-inverse on EVERY robot (two kernels) instead of
 *                                         the certifying one-launch step -- the A/B the equality test of the two is built on
 * Further A/B knobs (RMP2_PRIO_TAIL, RMP2_HEX_WAVES, RMP2_QUAD_LATENCY_BLOCKS) exist only in builds compiled with
 * -DRMP2_TUNING (tools/); the shipped library ignores them.  A deployment should leave all of them unset. */

/* Build an engine for one robot type + one RMP set on HIP device `device`.
 * Replaces: UrdfForwardKinematic.__init__ tables (kinematics.py:157-209) + the RmpCore
 * registry contents (rmp.py:114-131) as a flat, immutable "program".               */
int rmp2_create(const rmp2_desc *desc, int device, rmp2_handle **out);
int rmp2_destroy(rmp2_handle *h);

/* Last error message of `h` (or of the last failed rmp2_create when h == NULL). */
const char *rmp2_last_error(const rmp2_handle *h);

/* Name of the kernel (mapping of robots to lanes) the last rmp2_step / rmp2_rollout on `h` launched: which of the
 * three mappings runs is decided per call from the fleet size and the RMP set.  Diagnostic:
 * benchmarks and profiles name the kernel they measured from this instead of restating the dispatch rule. */
const char *rmp2_last_kernel(const rmp2_handle *h);

/* Stream-ordering fences for the obstacle exchange of a sharded fleet (fleet.py ObstacleExchange; the reference has
 * no counterpart -- its environment is a host-side list, rmp.py:264-315 reads it in Python).  A fence is a HIP event
 * WITHOUT timing and WITHOUT the system-scope release a default event carries: between two kernels of one stream a
 * default event's record costs ~7 us on MI355X (L2 write-back + the next kernel's cold start), a device-scope one
 * orders the same work for ~1 us.  Valid for work that stays on one GPU (the step kernel reading a table the RCCL
 * kernel of the same device wrote, and the write-after-read the other way); host-visible results still need an
 * ordinary event or a stream synchronisation.  `stream` is a hipStream_t (NULL = default stream). */
int rmp2_fence_create(int device, void **fence);
int rmp2_fence_record(void *fence, void *stream);          /* fence = everything enqueued on `stream` so far */
int rmp2_fence_wait(void *fence, void *stream);            /* later work on `stream` waits for the fence      */
int rmp2_fence_destroy(void *fence);
/* Attach `fence` to the handle: every later rmp2_step / rmp2_rollout on `h` signals it when its kernel completes -- the
 * effect of rmp2_fence_record right behind the launch, but carried by the dispatch itself (no extra packet between two
 * steps; ~3 us per step in the exchange loop).  NULL detaches.  A launch with a fence attached is not stream-capturable.
 * While a fence is attached, rmp2_step / rmp2_rollout on that handle carry per-handle state (the attachment): they must
 * then be issued from ONE thread at a time (handles stay independent of each other).  rmp2_fence_destroy refuses a fence
 * that is still attached (RMP2_ERR_INVALID_ARGUMENT); rmp2_destroy detaches. */
int rmp2_set_step_fence(rmp2_handle *h, void *fence);

/* Native obstacle exchange for a fleet sharded over the GPUs of a node (the `rmp2_comm_init` of SURVEY 8(b)):
 * every rank owns `spheres_per_rank` rows of the shared sphere table, the table [nranks * spheres_per_rank][4] is
 * all-gathered once per control step with RCCL on the exchange's own stream, double-buffered and one step ahead of the
 * kernel that consumes it; gather, stream orderings and the step launch are ONE call per control step (the same loop
 * driven from Python through torch.distributed costs ~50 us of host time per step, more than the step kernel takes).
 * RCCL is bound at run time: `rccl_library` is the path of the librccl.so the process uses (e.g. PyTorch's own copy), so
 * this library has no link-time dependency on it.  Rank 0 calls rmp2_exchange_unique_id and ships the 128 bytes to the
 * other ranks by any means (bench.py: torch.distributed broadcast); every rank then calls rmp2_exchange_create
 * (collective: it returns when all `nranks` ranks have joined).  One issuing thread per exchange. */
typedef struct rmp2_rccl_uid { char bytes[128]; } rmp2_rccl_uid;  /* ncclUniqueId */
typedef struct rmp2_exchange rmp2_exchange;
int rmp2_exchange_unique_id(const char *rccl_library, rmp2_rccl_uid *uid);
int rmp2_exchange_create(const char *rccl_library, const rmp2_rccl_uid *uid, int rank, int nranks, int device,
                         int spheres_per_rank, rmp2_exchange **out);
int rmp2_exchange_destroy(rmp2_exchange *x);
const char *rmp2_exchange_last_error(const rmp2_exchange *x);
int rmp2_exchange_pending(const rmp2_exchange *x);
/* Ranks of the communicator this exchange joined: ncclCommCount of the communicator itself, queried at create time -- which
 * also REFUSES a communicator whose ncclCommCount / ncclCommUserRank differ from the (rank, nranks) it was asked to join with --;
 * the `nranks` of the call only where the collective library does not export the two queries; 0 for NULL. */
int rmp2_exchange_nranks(const rmp2_exchange *x);
/* Pipeline depth (before the first rmp2_exchange_start): depth + 1 gathers may be outstanding.  1 (default): the table of step
 * k is gathered from slices produced before step k - 1 was issued -- the obstacles a step sees are ONE control step old, as in
 * the reference's loop, which re-reads the obstacle data every control step (06_cluttered_environment.py:120-131).  2: one more
 * control step of staleness and one more step of slack for the gather.  THREE table buffers rotate at either depth: the gather
 * for step k + 1, issued with the launch of step k, lands in a buffer whose last reader was step k - 2 -- long complete -- and so
 * starts at once and has a whole step to find a CU beside the running kernel (which fills every SIMD; with two buffers it had
 * to wait for step k - 1 and regularly made step k + 1 wait: 49.7 against 41.6 us per step at 65 536 robots,
 * profiles/r04_exchange_timing.txt).  RMP2_EXCHANGE_BUFFERS=2 (diagnostic) restores depth + 1 buffers. */
int rmp2_exchange_set_depth(rmp2_exchange *x, int32_t depth);   /* gathers started and not yet consumed by a step (0 .. 2) */
/* on != 0: a one-rank exchange orders its steps as an N-rank one does (GPU-side wait on the gathered table kept): what a
 * single-GPU EMULATION of an N-rank run must time.  No effect at nranks > 1 (the wait is always kept there). */
int rmp2_exchange_set_peer_wait(rmp2_exchange *x, int32_t on);
/* Issue the all-gather of `local` (device [spheres_per_rank][4]) into the free table buffer; it waits for the last step
 * that read the buffer it overwrites and -- local_is_ready == 0 -- for everything enqueued on `stream` so far (the producer
 * of `local`).  local_is_ready != 0: the caller guarantees that `local` is complete when this call is made (produced by an
 * earlier, already synchronised step of its pipeline, or static): no event is put on `stream`.  At most depth + 1 gathers may
 * be outstanding. */
int rmp2_exchange_start(rmp2_exchange *x, const float *local, int32_t local_is_ready, void *stream);
/* One control step (as rmp2_step with SHARED_SPHERES) on the OLDEST outstanding table.  next_local != NULL: the gather of
 * the next table is issued before the launch (same as rmp2_exchange_start(x, next_local, next_local_is_ready, stream)) --
 * or right behind it, ordered after this step's read, when all depth + 1 buffers were outstanding and the gather therefore
 * lands in the buffer this very step reads.
 * table_out (optional): device pointer of the table this step reads. */
int rmp2_exchange_step(rmp2_exchange *x, rmp2_handle *h, const float *q, const float *qd, const float *goal,
                       int32_t goal_stride, const float *next_local, int32_t next_local_is_ready, const rmp2_outputs *out,
                       int32_t R, void *stream, const float **table_out);

/* Pre-size the per-handle device buffers a step of up to R robots needs, so that rmp2_step never allocates.  Only handles whose
 * step is TWO kernels own such a buffer: solve = PINV sets without an inertia leaf and rank-deficient sets under AUTO (the
 * combined metric / force of every robot between the quad mapping and rmp2_pinv_kernel, 8 n (n + 1) bytes per robot); every
 * other handle: no-op.  Without it the first step of a larger fleet grows the buffer (hipFree + hipMalloc: a device
 * synchronisation, refused with RMP2_ERR_UNSUPPORTED while the stream is being captured).  Such a handle carries that buffer as
 * per-handle state: its steps must be issued on ONE stream at a time. */
int rmp2_reserve(rmp2_handle *h, int32_t R);

/* One control step for R robots: qdd = resolve(sum_i pullback(leaf_i))   (rmp.py:133-155).
 *   q, qd       device [R][n_dof] fp32
 *   goal        device [R][goal_floats] (goal_stride = goal_floats) or one shared row
 *               (goal_stride = 0); may be NULL when no leaf has a goal.
 *   obs         obstacle data (host struct holding device pointers); NULL = RMP2_OBS_NONE
 *   stream      hipStream_t (NULL = default stream); the call is asynchronous.          */
int rmp2_step(rmp2_handle *h, const float *q, const float *qd, const float *goal, int32_t goal_stride,
              const rmp2_obstacles *obs, const rmp2_outputs *out, int32_t R, void *stream);

/* Closed-loop rollout of the fleet inside ONE launch (the reference's control loop
 * experiments/franka_panda/06_cluttered_environment.py:120-131 with simulation.step tracking qdd):
 *   repeat n_control_steps times:  qdd = control step(q, qd);
 *                                  repeat substeps times:  qd += dt * qdd;  q += dt * qd;
 * q and qd (device, [R][n_dof]) are advanced IN PLACE; out->qdd receives the last qdd, out->status the
 * OR of the per-step status words.  Goals and the sphere table are constant during the rollout;
 * RMP2_OBS_EXPLICIT_PAIRS is rejected (closest-point pairs are only valid for the state they were
 * computed at; sets with attached-point leaves roll out when their pairs come from a SHARED_SPHERES table with
 * link_capsules -- formed anew every control step inside the launch -- instead of explicit arrays).  A handle created with
 * RMP2_SOLVE_PINV rolls out with the pseudo-inverse semantics on every robot and step (certifying elimination + Jacobi for the
 * rest where the set has an inertia leaf; otherwise the 16-lanes-per-robot mapping's Jacobi at any fleet size;
 * RMP2_ERR_UNSUPPORTED where that mapping cannot hold the program) -- never resolved differently from what was asked for. */
typedef struct rmp2_rollout_cfg {
  int32_t n_control_steps;
  int32_t substeps;
  float dt;
  int32_t table_steps; /* obstacle motion inside the rollout (the reference re-reads the obstacle data every control step,
                          06_cluttered_environment.py:120-131): 0 or 1 = one table for all control steps; n_control_steps =
                          one table per control step, obs->spheres then holds [n_control_steps][n_spheres][4 (spheres) or 8
                          (capsules)] and control step k reads table k (sphere modes only; ragged lists index every table) */
} rmp2_rollout_cfg;

int rmp2_rollout(rmp2_handle *h, float *q, float *qd, const float *goal, int32_t goal_stride,
                 const rmp2_obstacles *obs, const rmp2_rollout_cfg *cfg, const rmp2_outputs *out, int32_t R,
                 void *stream);

/* Closest-point preprocessing as a stand-alone stage (the reference's calculate_distances,
 * simulation.py:462-484, which fills the Datamanager arrays read by taskmap.py:115-138).
 * `table` must be a SHARED_SPHERES table (either primitive) with K records.  For the i-th
 * FK_DISTANCE leaf (leaf order) and record k, pair index i*K + k:
 *   p_link[r][i*K + k][3] = origin of the leaf's frame (the control point),
 *   p_obs [r][i*K + k][3] = nearest point on the surface of primitive k.
 * The two arrays are a valid EXPLICIT_PAIRS input (pair_begin[l] = i*K); feeding them back
 * reproduces the fused table mode.  p_link / p_obs: device [R][n_distance_leaves*K][3].   */
int rmp2_closest_points(rmp2_handle *h, const float *q, const rmp2_obstacles *table, float *p_link, float *p_obs,
                        int32_t R, void *stream);
/* The same stage with LINK GEOMETRY: the reference's control points are PyBullet's closest points on the link's collision
 * SHAPE, different for every (link, obstacle) pair (simulation.py:462-484 -> data_management.py:22-37), not the frame
 * origin.  link_capsules: device [n_distance_leaves][8] = (a.xyz, radius, b.xyz, unused), the link of the i-th distance leaf
 * as a capsule in that leaf's FRAME coordinates (urdf.py link_capsules: from the URDF's primitive collision geometry, or
 * supplied by the caller for mesh links).  Per pair: the nearest points of the link capsule's and the obstacle primitive's
 * surfaces (capsule-vs-sphere, capsule-vs-capsule).  link_capsules == NULL: rmp2_closest_points. */
int rmp2_closest_points_links(rmp2_handle *h, const float *q, const rmp2_obstacles *table, const float *link_capsules,
                              float *p_link, float *p_obs, int32_t R, void *stream);

/* ---- self collision: link-vs-link pairs formed on the device ---------------------------------------------------------
 * The reference's self-avoidance data path (simulation.py:411-441 with helper/pybullet_helper.py:46-68; switched off there at
 * simulation.py:406): every link A that carries a distance or attached-point leaf is paired with every other link B that has a
 * collision shape -- the fixed base included -- unless one is within 3 parent hops of the other (urdf.self_collision_pairs).
 * "linkB is interpreted as obstacle": a self pair is one more entry in A's leaf's pair range, with the values and the derivative
 * rule of an obstacle pair of that leaf (FK_DISTANCE: d = |p_link - p_obs|, derivative through the frame origin, quirk Q5;
 * FK_POINT: the attached point with its lever arm).  No derivative flows through B; there is no two-body Jacobian.
 *
 * rmp2_set_self_collision: copy the pair list into the handle.  pairs (host) [n_pairs][2] = (descriptor leaf index of an
 * FK_DISTANCE or FK_POINT leaf, frame B or -1 = the base link); capsules (host) [n_frames + 1][8] = (a.xyz, radius, b.xyz, -)
 * per frame in FRAME coordinates, the last row the base link in base coordinates (urdf.self_collision_capsules).  A leaf's pairs
 * keep the order given; leaves in descriptor order.  n_pairs == 0 or pairs == NULL turns the feature off: the handle then steps
 * exactly as one on which this was never called.  At most RMP2_MAX_SELF_PAIRS pairs; B must differ from the leaf's own frame.
 * Synchronous (one small host-to-device copy).
 *
 * rmp2_self_pairs: the stand-alone stage.  Per robot, leaf ordinal i's pairs (i-th pair-consuming leaf in descriptor order)
 * at [S_0 + ... + S_{i-1}, + S_i), S_l = pairs of leaf l:
 *   FK_DISTANCE leaf: p_link, p_obs = the nearest points of the two capsule SURFACES in the base frame;
 *   FK_POINT leaf:    p_link = relative_position (the point on A's surface in A's joint frame), p_obs = unit normal (base frame),
 *                     dist = distance (data_management.py:33-53), as rmp2_device.h link_pair_fields forms them for a table.
 * p_link, p_obs device [R][S][3]; dist device [R][S] (required when an attached-point leaf has self pairs, else may be NULL).
 * Intersecting capsule axes take the fixed normal +z (finite).  Feeding the arrays to an EXPLICIT_PAIRS step reproduces what
 * rmp2_step does with self collision on and no obstacle table.  A NaN or an infinity in one robot's q stays in that robot's rows:
 * every other robot's rows keep their bits (the staged step answers such a robot with a non-finite qdd and RMP2_STATUS_NONFINITE).
 *
 * rmp2_step on a handle with self collision: the stage, then the explicit-pair step (two launches).  Obstacle input NONE, or
 * SHARED_SPHERES with sphere or capsule records (with or without link_capsules) on sets without attached-point leaves: leaf l's
 * range is then [K obstacle pairs | S_l self pairs], the obstacle half bit-identical to rmp2_closest_points_links on the same
 * inputs (its default wave form).  Memory: the handle's stage buffer, here 24 P (+ 4 P with attached-point leaves) bytes per
 * robot, P = sum over the pair leaves of (K + S_l) -- config 3 with 32 spheres and 44 self pairs: 7 200 B per robot, 472 MB at
 * 65 536 robots.  A handle has ONE stage buffer, shared by its staged routes (self collision, link hulls, link_capsules beyond the
 * fused limits: at most one runs per step); its size depends on the route in use.  It grows on demand to the largest need seen
 * (refused with the byte count when it exceeds the free device memory, and inside a stream capture: step once outside it first),
 * so a graph captured on a staged step stays valid only until the buffer grows -- on this route or another.  RMP2_ERR_UNSUPPORTED, with a message naming the combination: RAGGED_SPHERES lists, CYLINDER
 * tables, caller-supplied EXPLICIT_PAIRS, a table with attached-point leaves, rmp2_rollout, rmp2_step_pair and
 * rmp2_exchange_step.  Out of scope: those forms, a symmetric (two-body) self-pair Jacobian, mesh-exact distances (capsules
 * stand in, as for obstacles). */
int rmp2_set_self_collision(rmp2_handle *h, int32_t n_pairs, const int32_t *pairs, const float *capsules);
int rmp2_self_pairs(rmp2_handle *h, const float *q, float *p_link, float *p_obs, float *dist, int32_t R, void *stream);

/* ---- convex-hull link geometry: closest points on the collision meshes ----------------------------------------------
 * The reference's closest points are PyBullet's, between the link's collision MESH -- loaded as its convex hull -- and the
 * obstacle (simulation.py:462-484 -> data_management.py:22-53).  Capsules contain their mesh, so rmp2_closest_points_links
 * under-estimates every distance; a handle with link hulls uses the hulls themselves (urdf.link_hulls).
 *
 * rmp2_set_link_hulls: copy one convex hull per pair leaf (the FK_DISTANCE and FK_POINT leaves, descriptor order) into the
 * handle.  Host arrays: hull i has the vertices verts[vert_offset[i] .. vert_offset[i+1])[3] and the face planes
 * planes[face_offset[i] .. face_offset[i+1])[4] = (n, d), n a unit outward normal, n . x <= d inside, all in the leaf's FRAME
 * coordinates (vert_offset[0] = face_offset[0] = 0).  At most RMP2_MAX_HULL_VERTICES vertices and RMP2_MAX_HULL_FACES planes per
 * hull (RMP2_ERR_INVALID_ARGUMENT beyond).  Synchronous.  n_hulls == 0 turns the feature off: the handle then steps bit for bit
 * as one on which this was never called.
 *
 * rmp2_closest_points_hulls: the stand-alone stage for a SHARED_SPHERES table of K sphere or capsule records.  Pair leaf i
 * owns pairs [i*K, (i+1)*K) (for sets without attached-point leaves the layout of rmp2_closest_points_links).  Per pair, with
 * c the obstacle's axis point -- the sphere centre, or the point of the capsule's segment the GJK iteration picks -- and r its
 * radius, in the leaf's frame (the obstacle is brought there as R^T (x - t), so the hull is one constant for the fleet):
 *   axis outside the hull: h = the hull point nearest the axis, n = (c - h) / |c - h|; p_link = h, p_obs = c - r n (also a sphere
 *     that overlaps the hull while its centre stays outside);
 *   axis meets the hull (the centre inside, the segment piercing it, or within 1e-7 m of its surface): the separating face of
 *     least translation over the hull's planes, t_f = d_f - min over the segment's endpoints of n_f . x, f* = argmin t_f, x* the
 *     endpoint attaining that min; p_link = x* + t_f* n_f*, p_obs = x* - r n_f*.  Conservative against PyBullet's EPA, which
 *     also weighs edge-edge directions.  The gap therefore JUMPS where a capsule's axis grazes an edge: on the unit cube [0, 1]^3
 *     the axis (0.5, 0.5, 1.5)-(1.5, 0.5, 0.5) touches the edge x = z = 1 at (1, 0.5, 1) and no face separates it from the cube
 *     by less than 0.5 (the faces +x and +z tie), so g = -(0.5 + r); the same axis 2e-7 m further out is apart, g = 2e-7 - r.  A
 *     step of half the hull's width across the 1e-7 m touch threshold, by the rule; the distance itself is continuous there.
 *   FK_DISTANCE leaf: p_link, p_obs in the base frame (explicit-pair semantics: d = |p_link - p_obs|, the derivative follows
 *     the frame origin, quirk Q5).
 *   FK_POINT leaf: the fields rmp2_device.h link_pair_fields forms from the same two points: p_link = relative_position (the
 *     hull point in the joint frame), p_obs = normal_vec = sign(g) u (base frame) and dist = |g|, where u is the unit direction
 *     from c to the hull point (-n_f* when the axis meets the hull) and g the signed gap (|h - c| - r outside, -(t_f* + r) when
 *     the axis meets the hull).
 * p_link, p_obs device [R][L*K][3]; dist device [R][L*K] (|g| for every pair; required when the set has attached-point leaves,
 * else it may be NULL).  The device iteration is bounded: at most 32 GJK steps per pair (fp64), one pass over the planes.
 * Non-finite inputs: a NaN or an infinity ANYWHERE in an obstacle record (centre or endpoints, radius, a capsule record's unused
 * float) makes p_link, p_obs and dist of that record's pairs NaN for every robot and every leaf, and leaves every other pair's
 * bits alone; a NaN or an infinity in a robot's q makes every pair output of that robot NaN, the leaves upstream of the joint
 * included, and leaves the other robots' bits alone.  Never a finite distance, never +-inf beside finite points.  The step that
 * follows turns such a pair into NaN on every joint of the robots that hold it, with RMP2_STATUS_NONFINITE.
 *
 * rmp2_step on a handle with hulls and a SHARED_SPHERES sphere / capsule table: this stage into a buffer of the handle, then the
 * explicit-pair step (two launches; the same numbers as calling the two).  Memory: the handle's stage buffer (rmp2_set_self_collision),
 * here 24 P (+ 4 P with attached-point leaves) bytes per robot, P = L*K; grown on demand, refused with the byte count beyond the
 * free device memory and inside a stream capture (step once outside it first).  The handle keeps one set of hull arrays, for
 * whichever hull geometry is on: these hulls, or those of rmp2_set_self_collision_hulls.  Obstacle input NONE, or an empty table,
 * steps as without hulls.
 * RMP2_ERR_UNSUPPORTED, with a message naming the combination: rmp2_rollout, rmp2_step_pair, rmp2_exchange_step, RAGGED_SPHERES
 * lists, CYLINDER tables, caller-supplied EXPLICIT_PAIRS, link_capsules given together with hulls, hulls together with self
 * collision (hull self pairs: rmp2_set_self_collision_hulls).  Out of scope: cylinder obstacles. */
int rmp2_set_link_hulls(rmp2_handle *h, int32_t n_hulls, const int32_t *vert_offset, const float *verts, const int32_t *face_offset,
                        const float *planes);
int rmp2_closest_points_hulls(rmp2_handle *h, const float *q, const rmp2_obstacles *table, float *p_link, float *p_obs, float *dist,
                              int32_t R, void *stream);

/* ---- hull-versus-hull self pairs: the reference's full distance state on the collision meshes ----------------------------
 * The reference asks PyBullet for link-vs-obstacle AND link-vs-link closest points, both on the links' collision meshes loaded as
 * convex hulls (simulation.py:411-484).  rmp2_set_self_collision_hulls is rmp2_set_self_collision with hulls in place of the
 * capsules: the same pairs (leaf ordinal's link A against frame B's link, an obstacle for the step; urdf.self_collision_pairs), and
 * n_hulls == n_frames + 1 entries packed as for rmp2_set_link_hulls -- entry f is frame f's link in FRAME coordinates, the last the
 * base link in base coordinates (urdf.self_collision_hulls).  An entry may be empty (no vertices, no planes) only when no pair names
 * its frame as A or B; with an obstacle table every pair leaf needs one.  Limits and argument checks as rmp2_set_link_hulls
 * (RMP2_ERR_INVALID_ARGUMENT naming the limit).  Synchronous.  The hulls go to the handle's one set of hull arrays, which
 * rmp2_set_link_hulls uses too (the two geometries exclude each other).
 *   n_pairs == 0 (or rmp2_set_self_collision(h, 0, ...)) turns self collision off, either geometry: the handle then steps bit
 *   for bit as a fresh one.  rmp2_set_self_collision with capsules replaces the hulls and this call replaces the capsules.
 *   RMP2_ERR_UNSUPPORTED on a handle with link hulls; rmp2_set_link_hulls is refused on a handle with hull self pairs.
 * Per self pair, both hulls in A's frame (B placed by R_A^T R_B, R_A^T (p_B - p_A)):
 *   separated: GJK on the Minkowski difference A - B (B's support in direction d taken in B's own coordinates against
 *     R_AB^T d), h_A and h_B the nearest points, g = |h_A - h_B|, u = (h_A - h_B) / g; p_link = h_A, p_obs = h_B.
 *   overlapping or touching (|v|^2 <= 1e-14, or a GJK tetrahedron holding the origin): over the face normals n of A and the
 *     negated face normals of B, s(n) = min_{y in B} n . y - max_{x in A} n . x (the plane offset d for the hull's own faces);
 *     n* = argmax s (A's faces first, the first maximum), y* the vertex of B attaining the min; p_obs = y*, p_link = y* - s n*,
 *     g = s < 0, u = -n*.  Edge-edge axes are not weighed: conservative against PyBullet's EPA, and unpinned (no reference depths).
 *     Where n* is a face of B, every vertex of that face attains the min: y* is one of them, which one is left to rounding.
 *   Either way p_link - p_obs = g u.  FK_DISTANCE leaves: both points in the base frame.  FK_POINT leaves: p_link =
 *   relative_position (h_A in the joint frame), p_obs = normal_vec = sign(g) u (base frame), dist = |g|.  u is found in A's frame
 *   and turned into the base frame by R_A: normal_vec is in base coordinates however far A's frame has turned.
 *   Bounded: at most 64 GJK steps per pair (fp64; the best simplex is kept), one pass over each hull's planes for the face rule.
 *   Non-finite inputs: a NaN or an infinity in a robot's q makes p_link, p_obs and dist of EVERY self pair (and every obstacle
 *   pair: rmp2_closest_points_hulls' contract) of that robot NaN, whichever frames the pair names, and leaves the other robots'
 *   bits alone.  Never a finite distance, never +-inf beside finite points.
 * rmp2_self_pairs on such a handle gives the hull pairs (layout of rmp2_set_self_collision).  rmp2_step with obstacle input NONE
 * or a SHARED_SPHERES sphere / capsule table: each pair leaf's range is [K obstacle pairs | S_l self pairs], the obstacle pairs
 * formed on the same leaf hulls, bit-identical to rmp2_closest_points_hulls on a handle whose link hulls are those hulls; then
 * the explicit-pair step.  A pair leaf without self pairs (S_l == 0) keeps its K obstacle pairs alone.  Two pair leaves on one
 * frame are two leaves: each has its own self pairs and its own K obstacle pairs on that frame's hull, and equal (frame, B) pairs
 * give equal rows.  Buffer, growth and capture refusals as rmp2_set_self_collision's staged step.  RMP2_ERR_UNSUPPORTED,
 * naming the combination: rmp2_rollout, rmp2_step_pair, rmp2_exchange_step, RAGGED_SPHERES lists, CYLINDER tables,
 * caller-supplied EXPLICIT_PAIRS, link_capsules given, a table on a set with attached-point leaves. */
int rmp2_set_self_collision_hulls(rmp2_handle *h, int32_t n_pairs, const int32_t *pairs, int32_t n_hulls, const int32_t *vert_offset,
                                  const float *verts, const int32_t *face_offset, const float *planes);

/* ---- inverse dynamics: the joint torques that realise the policy's q'' ----------------------------------------------------
 * The reference drives its robot in TORQUE_CONTROL with p.calculateInverseDynamics(q, qd, qdd) of the policy's q''
 * (simulation.py:369-386).  rmp2_inverse_dynamics gives, per robot, the generalised forces tau at which the fixed-base tree reaches
 * the accelerations qdd at the state (q, qd) under gravity g:
 *   tau = M(q) qdd + C(q, qd) qd + G(q),
 * the rigid-body model of the inertial table (no joint damping or friction, no limits, no rotor inertia).  tau_j is the torque
 * about the joint axis z_j of a revolute joint, the force along z_j of a prismatic one.  tau[R][n_dof] is in the caller's q order;
 * fixed joints have no entry; a movable joint missing from the joint order (q_index = -1) is held at q = qd = qdd = 0 and has no
 * entry, as in the FK.  The fixed base link's own inertia plays no part.  The robots stand at the base-frame origin; g is given
 * in the base frame.
 *
 * rmp2_set_inertials: copy the inertial table into the handle.  inertials: host [n_frames][10], frame f's record describing the
 * link that moves with frame f (the joint's child link) in FRAME coordinates: (m, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Ixz, Iyz), c the
 * centre of mass and the tensor taken about c in frame axes (the URDF's ixy etc. as matrix entries; urdf.inertial_table builds
 * it from the <inertial> elements).  gravity: host [3], or NULL for (0, 0, -9.81) (p.setGravity, simulation.py:329).  Synchronous.
 * n_frames == 0 switches the feature off.  RMP2_ERR_INVALID_ARGUMENT, naming the frame: a frame count other than the robot's, a
 * non-finite value, m < 0, a negative diagonal moment; also a non-finite gravity.
 *
 * rmp2_inverse_dynamics: q, qd, qdd device [R][n_dof], tau device [R][n_dof]; stream-ordered, no host synchronisation and no
 * allocation (it can be captured in a graph).  R == 0 is a no-op.  Refused (RMP2_ERR_INVALID_ARGUMENT) without inertials.
 * Inputs and tau are fp32; a NaN or Inf in a robot's q, qd or qdd gives a non-finite tau for that robot and leaves the others
 * unaffected.  One forward walk per robot over every frame (csrc/rmp2_dynamics.h); rmp2_step, rmp2_forward_kinematics and
 * rmp2_rollout are untouched by the table.
 *
 * Where this departs from PyBullet: the reference loads its URDFs without URDF_USE_INERTIA_FROM_FILE, and PyBullet then replaces
 * the file's inertia tensors by an approximation from the collision shape; the engine uses the table the caller gives (urdf
 * builds it from the file).  Parity with the reference's torques is UNPINNED: no PyBullet result backs these numbers; the tests
 * pin them against two independent fp64 derivations (Newton-Euler and Lagrangian). */
int rmp2_set_inertials(rmp2_handle *h, int32_t n_frames, const float *inertials, const float *gravity);
int rmp2_inverse_dynamics(rmp2_handle *h, const float *q, const float *qd, const float *qdd, float *tau, int32_t R, void *stream);

/* ---- forward dynamics: the plant that answers the torques --------------------------------------------------------------------
 * After the torques the reference calls p.stepSimulation: the robot's own equations of motion answer them.  These three entry
 * points are that half for a fleet, on the model of rmp2_inverse_dynamics: the rigid bodies of the inertial table, a fixed base,
 * the gravity of rmp2_set_inertials; no damping, friction, rotor inertia, joint limits or contacts (joint-limit stops: the block
 * after this one, rmp2_dynamics_step_stops; obstacle contacts: the one after that, rmp2_dynamics_step_contacts).  With
 * tau_id(a) = M(q) a + C(q, qd) qd + G(q), one routine serves both drives:
 *     qdd = qdd_in + M(q)^-1 (tau_applied - tau_id(qdd_in))
 *   torque drive:        qdd_in = 0, tau_applied = the caller's tau:  qdd = M^-1 (tau - C qd - G);
 *   acceleration drive:  qdd_in = qdd_des, tau_applied = clamp(tau_id(qdd_des), +-tau_limit) (what simulation.step does).  With
 *                        no limit, or where no joint of a robot saturates, tau_applied - tau_id is exactly zero, the solve is
 *                        skipped and the robot's qdd is qdd_des bit for bit.
 *
 * rmp2_mass_matrix: q device [R][n_dof]; M device [R][n_dof][n_dof], symmetric, both triangles written from one computed
 * triangle (the counterpart of p.calculateMassMatrix).  rmp2_forward_dynamics: q, qd, tau device [R][n_dof] -> qdd.
 * rmp2_dynamics_step: the plant's step, in place:  repeat substeps times:
 *     qdd = the solve above;  qd += dt * qdd;  q += dt * qd;          (the integrator of rmp2_rollout)
 *   drive = RMP2_DRIVE_TORQUE: u = tau, held over the substeps, clamped by tau_limit if given;
 *   drive = RMP2_DRIVE_ACCEL : u = qdd_des, held over the substeps; tau recomputed at every substep's state
 *                              (simulation.py:369-381).
 *   tau_limit: device [n_dof], >= 0 (+inf = no limit on that joint), shared by the fleet, or NULL.
 *   qdd_out / tau_out: device [R][n_dof] or NULL, the last substep's qdd and applied tau.
 * All three are stream-ordered, without host synchronisation or allocation (they can be captured in a graph); R == 0 is a
 * no-op.  RMP2_ERR_INVALID_ARGUMENT with a message: a null array, R < 0, substeps < 1, a dt that is not finite or not > 0, an
 * unknown drive, and a handle without inertials (the message names rmp2_set_inertials).
 *
 * Edge behaviour:
 *   - a dof that no joint of the program owns takes no part in the system: its row of M is e_j and its qdd is 0 (in either
 *     drive; its entry of u is ignored);
 *   - a movable joint missing from the joint order is held at 0, as in the FK and the inverse dynamics;
 *   - M not numerically positive definite -- a Cholesky pivot <= 0 or not finite, e.g. a moving joint whose whole subtree is
 *     massless: every entry of that robot's qdd is NaN, and in rmp2_dynamics_step so are its q and qd; the other robots are
 *     unaffected; rmp2_mass_matrix still returns that robot's M.  (An acceleration drive in which nothing saturates never
 *     factors M and returns qdd_des.)
 *   - a non-finite value anywhere in a robot's input rows (q, qd, tau / u) makes every output of that robot NaN and leaves the
 *     others unaffected.
 * fp32 throughout: one forward walk per robot that sums tau_id and M together, then a Cholesky factorisation and two
 * triangular solves (csrc/rmp2_forward_dynamics.h).  rmp2_step, rmp2_forward_kinematics, rmp2_rollout and
 * rmp2_inverse_dynamics are untouched.  Parity with PyBullet's stepSimulation is UNPINNED, as for the inverse dynamics (PyBullet
 * replaces the file's inertia and adds default link damping); the tests pin these against fp64 restatements. */
#define RMP2_DRIVE_TORQUE 0
#define RMP2_DRIVE_ACCEL 1
int rmp2_mass_matrix(rmp2_handle *h, const float *q, float *M /* [R][n_dof][n_dof], symmetric, both triangles */, int32_t R, void *stream);
int rmp2_forward_dynamics(rmp2_handle *h, const float *q, const float *qd, const float *tau, float *qdd, int32_t R, void *stream);
int rmp2_dynamics_step(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive, const float *tau_limit,
                       float dt, int32_t substeps, float *qdd_out, float *tau_out, int32_t R, void *stream);

/* ---- joint-limit stops: the plant's step inside [q_lower, q_upper] -----------------------------------------------------------
 * rmp2_dynamics_step_stops is rmp2_dynamics_step with inelastic stops at the joint limits, acting at velocity level.  At a
 * substep's state (q, qd), with a the acceleration of the block above (either drive, tau_limit as there) and v* = qd + dt a,
 * every dof j that a joint owns has the velocity box
 *     l_j = min((lo_j - q_j) / dt, 0),   h_j = max((hi_j - q_j) / dt, 0)
 * (-inf / +inf limits: no bound; an unowned dof: no bound; a joint already outside its limits is not pushed back, it only cannot
 * move further out; lo_j == hi_j locks the joint once it is there).  The step's velocity is the box-constrained minimiser in
 * the kinetic-energy metric (Gauss' principle; the inelastic limit of what a constraint-impulse solver converges to):
 *     v = argmin 1/2 (v - v*)^T M(q) (v - v*)   subject to   l <= v <= h,
 * whose unique solution satisfies, with lambda = M (v - v*): lambda_j >= 0 where v_j = l_j, lambda_j <= 0 where v_j = h_j,
 * lambda_j = 0 on free dofs, any sign where l_j = h_j.  Then qd <- v, q <- q + dt v; in a substep that ran the solver a dof whose
 * bound came from its limit lands on the limit exactly and no rounding takes a joint that was inside its limits outside (a
 * substep on the fast path below integrates as rmp2_dynamics_step does, to one fp32 rounding).  Outputs of the last substep:
 *     qdd_out = a + (v - v*) / dt,   tau_out = the applied motor torque as above,   stop_out = lambda / dt (the stops' torque).
 *   q_lower / q_upper: device [n_dof], shared by the fleet, both required (lower <= upper; +-inf where there is no limit).
 *   stop_out: device [R][n_dof] or NULL.  status_out: device [R] or NULL: RMP2_STOP_* flags over the substeps, and in bits 8..
 *   the largest number of solver iterations a substep of that robot took.
 * Solver: the primal active-set method, one bound at a time, from v = clip(v*, l, h); every iterate is feasible and the
 * objective never increases, so the iteration cap leaves a valid in-limits velocity and is reported (RMP2_STOP_CAPPED).
 * A robot whose v* already lies in the box runs none of it: its q, qd, qdd_out and tau_out are those of rmp2_dynamics_step bit
 * for bit, its stop_out is exactly 0 and its status 0.
 * Stream-ordered, no allocation, capturable; refusals as for rmp2_dynamics_step, and null limit arrays ("null array").  The edge behaviour of
 * the block above holds unchanged (unowned dofs, missing joints, M not positive definite -> the robot's rows NaN, non-finite
 * input rows -> that robot NaN and the others untouched).  One lane per robot, M kept in LDS across the iterations
 * (csrc/rmp2_joint_stops.h); every other entry point is untouched.  Parity with PyBullet's constraint solver is UNPINNED, as
 * for the rest of the plant; the tests pin this against an fp64 restatement and against brute-force enumeration. */
#define RMP2_STOP_ACTIVE 1u   /* some stop was active in some substep */
#define RMP2_STOP_CAPPED 2u   /* the iteration cap was reached in some substep */
int rmp2_dynamics_step_stops(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive,
                             const float *tau_limit, const float *q_lower, const float *q_upper, float dt, int32_t substeps,
                             float *qdd_out, float *tau_out, float *stop_out, uint32_t *status_out, int32_t R, void *stream);

/* ---- obstacle contacts: the plant's step outside a table of spheres -----------------------------------------------------------
 * rmp2_dynamics_step_contacts is rmp2_dynamics_step_stops with frictionless, inelastic, velocity-level contacts between the
 * robot's link capsules (rmp2_set_contact_capsules: host [n_frames][8] = (a, radius, b, 0) in frame coordinates, a zero row =
 * no capsule; NULL or n_frames == 0 switches them off) and a STATIC table of spheres shared by the fleet (device [K][4] =
 * centre, radius; K <= 256).  Stops and contacts are solved together, one problem per substep.  At a substep's state (q, qd),
 * with a, v* = qd + dt a and the box (l, h) of the block above, for each frame f with a non-zero capsule row and each sphere k:
 *     X = the point of the capsule's world segment nearest the centre c_k;   n = (X - c_k) / |X - c_k|  (the fixed direction +z
 *     where the centre lies on the segment: link_normal_length's convention);   gap g = |X - c_k| - r_k - r_f;
 *     row J_fk[j] = n . (z_j x (X - o_j)) for a revolute ancestor dof j of f, n . z_j for a prismatic one, 0 otherwise (z_j, o_j:
 *     the joint's world axis and origin);   bound b_fk = -max(g, 0) / dt: a pair already in penetration is not pushed out, it
 *     only cannot go deeper -- the stops' rule.
 * The CANDIDATES of a robot in a substep are the pairs with g <= d_act (metres, finite, >= 0), at most RMP2_MAX_CONTACTS; when
 * more qualify the smallest gaps are taken, ties going to the lower pair index f K + k, and the excess is reported
 * (RMP2_CONTACT_OVERFLOW).  The substep's velocity is
 *     v = argmin 1/2 (v - v*)^T M(q) (v - v*)   s.t.   l <= v <= h,   J_c v >= b_c for every candidate c,
 * which is unique (v = 0 is always feasible) and satisfies M (v - v*) = sigma + sum_c lambda_c J_c^T, lambda_c >= 0,
 * lambda_c (J_c v - b_c) = 0, sigma as the block above's lambda.  CONTRACT: the result is the all-pairs solution whenever
 * d_act >= dt x the largest approach speed of a pair and nothing overflows.  Then qd <- v, q <- q + dt v with the stops' exact
 * landing and clamps.  Outputs of the last substep (each of the new ones may be NULL):
 *     qdd_out, tau_out as above;  stop_out = sigma / dt;  contact_out [R][n_dof] = sum_c lambda_c J_c^T / dt;
 *     contact_lambda [R][RMP2_MAX_CONTACTS] = lambda_c / dt, the normal force in N, 0 in empty slots;
 *     contact_pair [R][RMP2_MAX_CONTACTS] int32 = f K + k, -1 in empty slots (slots in no particular order);
 *     status_out: RMP2_STOP_ACTIVE, RMP2_STOP_CAPPED (the solver of stops or contacts stopped before optimality: the iteration
 *     cap, or a row refused because it depends on the working set to fp32 resolution; the velocity returned violates no
 *     constraint), RMP2_CONTACT_ACTIVE (some lambda_c > 0 in some substep), RMP2_CONTACT_OVERFLOW; iterations in bits 8.. .
 * Solver: primal active set over the rows +-e_j and J_c from v = 0; M factored once per substep, one column M^-1 a_i per
 * working row, the small Gram system solved every iteration (csrc/rmp2_contacts.h).  A substep in which a robot has no
 * candidate runs the block above's substep itself: a robot without a candidate in any substep gets rmp2_dynamics_step_stops'
 * results bit for bit with contact_* exactly 0 / -1, and with q_lower = q_upper = NULL (no limits) or limits far away
 * rmp2_dynamics_step's.  K == 0 is the stops call.  The block above's edge behaviour holds; a non-finite sphere record makes
 * every robot's outputs NaN.  Stream-ordered, no allocation, capturable.  Refusals as for the stops call (q_lower and q_upper
 * both given or both NULL), and: no capsules set, K < 0, K > 256, a null table with K > 0, d_act not finite or < 0; a robot
 * of more than 9 dofs: RMP2_ERR_UNSUPPORTED.  Friction, restitution, penetration recovery and moving obstacles are not
 * modelled (self contacts between the robot's own link capsules: rmp2_dynamics_step_contacts_self below); parity with PyBullet's solver is UNPINNED, as for the rest of the plant. */
#define RMP2_MAX_CONTACTS 8
#define RMP2_MAX_CONTACT_SPHERES 256
#define RMP2_CONTACT_ACTIVE 4u     /* some contact carried force in some substep */
#define RMP2_CONTACT_OVERFLOW 8u   /* more than RMP2_MAX_CONTACTS pairs qualified in some substep */
int rmp2_set_contact_capsules(rmp2_handle *h, int32_t n_frames, const float *capsules /* host [n_frames][8]; NULL or 0 = off */);
int rmp2_dynamics_step_contacts(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive, const float *tau_limit,
                                const float *q_lower, const float *q_upper /* both NULL = no limits */,
                                const float *spheres /* device [K][4] */, int32_t K, float d_act, float dt, int32_t substeps,
                                float *qdd_out, float *tau_out, float *stop_out, float *contact_out, float *contact_lambda,
                                int32_t *contact_pair, uint32_t *status_out, int32_t R, void *stream);

/* ---- obstacle contacts with per-robot lists over a shared pool of spheres -----------------------------------------------------
 * rmp2_dynamics_step_contacts_lists is rmp2_dynamics_step_contacts with every robot's own set of spheres: robot r's spheres are
 * spheres[csr_index[i]] for i in [csr_offset[r], csr_offset[r + 1]), in list order, out of a pool `spheres` (device [K][4],
 * 16-byte aligned, K <= RMP2_MAX_CONTACT_POOL).  csr_offset (device [R + 1]) and csr_index (device [csr_offset[R]]) have the
 * layout of rmp2_obstacles' fields of those names: the arrays built for rmp2_step's RMP2_OBS_RAGGED_SPHERES feed the plant
 * unchanged.  Everything else is the block above word for word: the pairs are (frame with a capsule, list entry); gap, normal,
 * row and bound; the candidates (g <= d_act, at most RMP2_MAX_CONTACTS, smallest gaps, ties to the lower pair index); solver,
 * landing, clamps, outputs and status flags.  contact_pair stays f K + k with K the POOL's size and k the POOL index (not the
 * position in the list).
 * Bit for bit: a robot with an empty list gets rmp2_dynamics_step_stops' results, contact_* exactly 0 / -1;  a robot whose list
 * is strictly ascending gets the results of rmp2_dynamics_step_contacts on the compacted table spheres[list] (status word
 * included), contact_pair f K' + k' becoming f K + list[k'] -- the evaluation order (frames outer, entries inner) and every
 * expression are the same code, and the tie order survives a monotone map.  A robot's results depend on no other robot's list,
 * not on R and not on its lane.  Unsorted lists: the same candidate set; slot order and bits may differ.  A repeated index is
 * two pairs with identical rows (as in the policy's ragged mode); both may take a slot.
 * INVALID lists are refused per robot, on the device (the host cannot see device arrays): a negative csr_offset[r], a negative
 * length, a length above RMP2_MAX_CONTACT_LIST, or an entry outside [0, K).  No record is read through a bad entry (every entry
 * is range-checked, once per launch, before anything is read through it); every output row of that robot is NaN, its
 * contact_pair -1 and its status_out exactly RMP2_CONTACT_LIST_INVALID; other robots are untouched.  That csr_index holds
 * csr_offset[r + 1] entries is the caller's contract, as for rmp2_step.  A non-finite record makes the robots that LIST it NaN
 * (the scan covers a robot's own entries, not the pool); the others are untouched.
 * Stream-ordered, no allocation, no host read-back of csr_offset: capturable.  Refusals as for rmp2_dynamics_step_contacts
 * except that the table's cap of 256 is the list's, not the pool's, and: csr_offset or csr_index NULL with R > 0, K < 0,
 * K > RMP2_MAX_CONTACT_POOL, a null or misaligned pool with K > 0; a robot of more than 9 dofs: RMP2_ERR_UNSUPPORTED.  K == 0
 * is accepted: every list must then be empty to be valid. */
#define RMP2_MAX_CONTACT_LIST 256          /* entries per robot */
#define RMP2_MAX_CONTACT_POOL (1 << 24)    /* records in the pool; 32 * K must fit the int32 pair index */
#define RMP2_CONTACT_LIST_INVALID 16u      /* status_out of a robot whose list was refused (alone: no other bit, no iterations) */
int rmp2_dynamics_step_contacts_lists(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive, const float *tau_limit,
                                      const float *q_lower, const float *q_upper /* both NULL = no limits */,
                                      const float *spheres /* device [K][4] */, int32_t K,
                                      const int32_t *csr_offset /* device [R+1] */,
                                      const int32_t *csr_index /* device [csr_offset[R]] */, float d_act, float dt,
                                      int32_t substeps, float *qdd_out, float *tau_out, float *stop_out, float *contact_out,
                                      float *contact_lambda, int32_t *contact_pair, uint32_t *status_out, int32_t R, void *stream);

/* ---- half-space obstacles (floor, walls) beside the spheres -------------------------------------------------------------------
 * rmp2_dynamics_step_contacts_planes is rmp2_dynamics_step_contacts (csr_offset == csr_index == NULL: spheres is the shared
 * table, K <= RMP2_MAX_CONTACT_SPHERES) or rmp2_dynamics_step_contacts_lists (both given: spheres is the pool) with a table of
 * half-spaces shared by the fleet: planes, device [P][4] fp32 = (nx, ny, nz, d), 16-byte aligned, 0 <= P <=
 * RMP2_MAX_CONTACT_PLANES; free space is {x : n . x >= d}.  A unit normal is the caller's contract: the record is used as given.
 * For each frame f with a capsule (world end points X_0 = A, X_1 = A + D, radius r_f), each plane p and each end e in {0, 1}:
 *     gap g = n . X_e - d - r_f;   J[j] = n . (z_j x (X_e - o_j)) (revolute ancestor dof j), n . z_j (prismatic), 0 otherwise;
 *     bound b = -max(g, 0) / dt   (a penetrating end is not pushed out; it cannot go deeper).
 * Two rows per capsule and plane, so that a link lying flat on a plane is held at both ends; a capsule of zero length (D == 0
 * exactly) gives the row e = 0 only.  Plane rows and sphere rows compete for the same RMP2_MAX_CONTACTS slots by the same rule
 * (g <= d_act, smallest gap first, ties to the lower pair index, the excess reported as RMP2_CONTACT_OVERFLOW).  The PAIR INDEX
 * of a plane row is F K + 2 (f P + p) + e, F the robot's frame count and K the sphere count (the pool's size in the list form):
 * sphere pairs keep f K + k and sort before plane pairs on ties; the RMP2_CONTACT_PAIR_* macros take a value apart.  Solver, status
 * flags, outputs, landing and clamps are those of the two calls above.
 * P == 0 is the sphere call;  K == 0 with P > 0 a planes-only step;  K == 0 and P == 0 the stops' step.  A non-finite plane
 * value makes every robot's outputs NaN (contact_pair -1), as a non-finite record of the shared sphere table does.
 * Stream-ordered, no allocation, no read-back: capturable.  Refusals: those of the call it extends, and P < 0, P >
 * RMP2_MAX_CONTACT_PLANES, a null or misaligned plane table with P > 0, one of csr_offset / csr_index without the other:
 * RMP2_ERR_INVALID_ARGUMENT; a robot of more than 9 dofs: RMP2_ERR_UNSUPPORTED. */
#define RMP2_MAX_CONTACT_PLANES 8
#define RMP2_CONTACT_KIND_SPHERE 0
#define RMP2_CONTACT_KIND_PLANE 1
/* contact_pair (>= 0) -> kind, frame, record, end.  F: the robot's frame count; K, P: the call's sphere and plane counts.  record is
 * the sphere's index (table or pool) or the plane's; end is the capsule's end point, 0 for a sphere. */
#define RMP2_CONTACT_PAIR_KIND(pair, F, K) ((int64_t)(pair) >= (int64_t)(F) * (K) ? RMP2_CONTACT_KIND_PLANE : RMP2_CONTACT_KIND_SPHERE)
#define RMP2_CONTACT_PAIR_PLANE_ROW(pair, F, K) ((int32_t)((int64_t)(pair) - (int64_t)(F) * (K))) /* 2 (f P + p) + e of a plane pair */
#define RMP2_CONTACT_PAIR_FRAME(pair, F, K, P) \
  (RMP2_CONTACT_PAIR_KIND(pair, F, K) ? (RMP2_CONTACT_PAIR_PLANE_ROW(pair, F, K) >> 1) / (P) : (pair) / (K))
#define RMP2_CONTACT_PAIR_RECORD(pair, F, K, P) \
  (RMP2_CONTACT_PAIR_KIND(pair, F, K) ? (RMP2_CONTACT_PAIR_PLANE_ROW(pair, F, K) >> 1) % (P) : (pair) % (K))
#define RMP2_CONTACT_PAIR_END(pair, F, K) (RMP2_CONTACT_PAIR_KIND(pair, F, K) ? RMP2_CONTACT_PAIR_PLANE_ROW(pair, F, K) & 1 : 0)
int rmp2_dynamics_step_contacts_planes(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive, const float *tau_limit,
                                       const float *q_lower, const float *q_upper, const float *spheres, int32_t K,
                                       const int32_t *csr_offset, const int32_t *csr_index, const float *planes, int32_t P,
                                       float d_act, float dt, int32_t substeps, float *qdd_out, float *tau_out, float *stop_out,
                                       float *contact_out, float *contact_lambda, int32_t *contact_pair, uint32_t *status_out,
                                       int32_t R, void *stream);

/* ---- capsule obstacles (posts, bars) beside the spheres and the half-spaces ------------------------------------------------------
 * rmp2_dynamics_step_contacts_capsules is rmp2_dynamics_step_contacts_planes (with or without csr_offset / csr_index) with a table
 * of capsule obstacles shared by the fleet: obstacle_capsules, device [C][8] fp32 = (a.xyz, radius, b.xyz, 0), 16-byte aligned,
 * 0 <= C <= RMP2_MAX_OBSTACLE_CAPSULES -- the record of RMP2_PRIM_CAPSULE tables.  There are no per-robot capsule lists.
 * For each frame f with a link capsule (world segment A, A + D, radius r_f) and each obstacle c = (C_0, r_c, C_1):
 *     (s, t) = the parameters of the nearest points of the two segments (A, A + D) and (C_0, C_1) -- the clamped 2 x 2 normal
 *              equations; parallel axes: the link's end s = 0 first --;   Y = C_0 + t (C_1 - C_0);
 *     from there the pair IS the sphere pair of rmp2_dynamics_step_contacts with centre Y and radius r_c, expression for expression:
 *     X = the point of the link's segment nearest Y, n = (X - Y) / |X - Y| (+z where they coincide: crossing axes),
 *     gap g = |X - Y| - r_c - r_f, the row J and the bound b = -max(g, 0) / dt as there.
 * One row per pair.  A capsule with a == b exactly is the sphere (a, radius).  Capsule rows compete for the RMP2_MAX_CONTACTS slots
 * with sphere and plane rows by the same rule.  The PAIR INDEX of a capsule row is F K + 2 F P + f C + c (F the robot's frame
 * count, K the sphere count -- the pool's size in the list form --, P the plane count): after every sphere and plane pair, so that
 * a tie goes to the earlier kind; at most 32 * 2^24 + 512 + 1024, within int32.  The RMP2_CONTACT_PAIR_CAPSULE_* macros take a
 * capsule pair apart, RMP2_CONTACT_PAIR_KIND3 tells the three kinds apart.
 * C == 0 is the planes call;  C == 0 and P == 0 the sphere or list call;  all of K, P, C zero the stops' step.  A non-finite value
 * anywhere in a capsule record makes every robot's outputs NaN (contact_pair -1), as for spheres and planes.
 * Limits: one row per pair -- a link lying ALONG a post (parallel axes) is held at one point per substep, the s = 0 end's
 * nearest point; flat-capped cylinders enter as capsules (urdf.cylinders_as_capsules on the Python side, with its stated bound).
 * Stream-ordered, no allocation, no read-back: capturable.  Refusals: those of rmp2_dynamics_step_contacts_planes, and C < 0,
 * C > RMP2_MAX_OBSTACLE_CAPSULES, a null or misaligned capsule table with C > 0: RMP2_ERR_INVALID_ARGUMENT. */
#define RMP2_MAX_OBSTACLE_CAPSULES 32
#define RMP2_CONTACT_KIND_CAPSULE 2
/* contact_pair (>= 0) of a call with C capsules -> kind; frame and record of a CAPSULE pair (the other kinds: the macros above) */
#define RMP2_CONTACT_PAIR_CAPSULE_BASE(F, K, P) ((int64_t)(F) * (K) + 2 * (int64_t)(F) * (P))
#define RMP2_CONTACT_PAIR_KIND3(pair, F, K, P) \
  ((int64_t)(pair) >= RMP2_CONTACT_PAIR_CAPSULE_BASE(F, K, P) ? RMP2_CONTACT_KIND_CAPSULE : RMP2_CONTACT_PAIR_KIND(pair, F, K))
#define RMP2_CONTACT_PAIR_CAPSULE_FRAME(pair, F, K, P, C) ((int32_t)(((int64_t)(pair) - RMP2_CONTACT_PAIR_CAPSULE_BASE(F, K, P)) / (C)))
#define RMP2_CONTACT_PAIR_CAPSULE_RECORD(pair, F, K, P, C) ((int32_t)(((int64_t)(pair) - RMP2_CONTACT_PAIR_CAPSULE_BASE(F, K, P)) % (C)))
int rmp2_dynamics_step_contacts_capsules(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive, const float *tau_limit,
                                         const float *q_lower, const float *q_upper, const float *spheres, int32_t K,
                                         const int32_t *csr_offset, const int32_t *csr_index, const float *planes, int32_t P,
                                         const float *obstacle_capsules /* device [C][8] */, int32_t C, float d_act, float dt,
                                         int32_t substeps, float *qdd_out, float *tau_out, float *stop_out, float *contact_out,
                                         float *contact_lambda, int32_t *contact_pair, uint32_t *status_out, int32_t R,
                                         void *stream);

/* ---- self contacts: the robot's own link capsules against each other -----------------------------------------------------------
 * rmp2_set_contact_self_pairs holds a list of unordered frame pairs {i, j} on the handle (host int32 [n_pairs][2]; n_pairs == 0:
 * self contacts off), like the link capsules of rmp2_set_contact_capsules and in any order against it; synchronous.
 * rmp2_dynamics_step_contacts_self is rmp2_dynamics_step_contacts_capsules -- its argument list, its refusals -- with one more
 * kind of row, one per pair.  Write anc(x) for the set of dofs that move frame x.  Of a pair the frame that the handle's full
 * program visits LATER (op order) is the link f, the other the partner e.  With the world segments (A_f, A_f + D_f, r_f) and
 * (A_e, A_e + D_e, r_e) of the two link capsules the pair IS the capsule pair above, expression for expression, the partner's
 * segment standing where the obstacle (C_0, C_1, r_c) stood:
 *     (s, t) = segment_segment(A_f, A_f + D_f, A_e, A_e + D_e);   Y = A_e + t D_e (formed from the segment's two ends);
 *     X = the point of f's segment nearest Y;   n = (X - Y) / |X - Y| (+z where they coincide);   g = |X - Y| - r_e - r_f;
 *     b = -max(g, 0) / dt;   a candidate when g <= d_act, competing for the RMP2_MAX_CONTACTS slots by the same rule.
 * The row:  J[j] = n . (z_j x (X - o_j)) (revolute; n . z_j prismatic) for j in anc(f) \ anc(e);
 *           J[j] = -n . (z_j x (Y - o_j)) (revolute; -n . z_j prismatic) for j in anc(e) \ anc(f);
 *           J[j] = 0 exactly for every other j, the dofs common to both links included (they move the pair rigidly).
 * On a serial chain anc(e) is a subset of anc(f): the one-body capsule row under the mask anc(f) & ~anc(e).
 * The PAIR INDEX of a self row is F K + 2 F P + F C + f F + e: after every sphere, plane and capsule pair, so that a tie goes
 * sphere, plane, capsule, self; at most 32 * 2^24 + 512 + 1024 + 1024 < 2^31.  The RMP2_CONTACT_PAIR_SELF_* macros take a self pair apart,
 * RMP2_CONTACT_PAIR_KIND4 tells the four kinds apart.
 * A pair on a frame whose link-capsule row is all zero is never a candidate, as for spheres.  With no pairs set the call is the
 * capsules call; with K = P = C = 0 as well the stops' step.
 * The setter refuses with RMP2_ERR_INVALID_ARGUMENT (the handle keeps the list it had): a frame out of range, i == j, a pair
 * given twice in either order, a pair with anc(i) == anc(j) (rigidly connected: its row would be identically zero), more than
 * RMP2_MAX_CONTACT_SELF_FRAMES distinct partner frames (the kernel keeps each partner's segment per robot: 22 x 6 words lie over
 * the solver's 135 words of a 9-dof robot, which are free during the search).
 * Limits: the static base link takes no part (its frame is not in the program); capsule against capsule, not hull against hull;
 * one row per pair -- parallel links are held at one point per substep; frictionless, inelastic, no position recovery; robots of
 * at most 9 dofs; no rollout fusion.  Stream-ordered, no allocation, no read-back: capturable. */
#define RMP2_MAX_CONTACT_SELF_FRAMES 22
#define RMP2_CONTACT_KIND_SELF 3
#define RMP2_CONTACT_PAIR_SELF_BASE(F, K, P, C) (RMP2_CONTACT_PAIR_CAPSULE_BASE(F, K, P) + (int64_t)(F) * (C))
#define RMP2_CONTACT_PAIR_KIND4(pair, F, K, P, C) \
  ((int64_t)(pair) >= RMP2_CONTACT_PAIR_SELF_BASE(F, K, P, C) ? RMP2_CONTACT_KIND_SELF : RMP2_CONTACT_PAIR_KIND3(pair, F, K, P))
#define RMP2_CONTACT_PAIR_SELF_LINK(pair, F, K, P, C) ((int32_t)(((int64_t)(pair) - RMP2_CONTACT_PAIR_SELF_BASE(F, K, P, C)) / (F)))
#define RMP2_CONTACT_PAIR_SELF_PARTNER(pair, F, K, P, C) ((int32_t)(((int64_t)(pair) - RMP2_CONTACT_PAIR_SELF_BASE(F, K, P, C)) % (F)))
int rmp2_set_contact_self_pairs(rmp2_handle *h, int32_t n_pairs, const int32_t *pairs /* host [n_pairs][2] */);
int rmp2_dynamics_step_contacts_self(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive, const float *tau_limit,
                                     const float *q_lower, const float *q_upper, const float *spheres, int32_t K,
                                     const int32_t *csr_offset, const int32_t *csr_index, const float *planes, int32_t P,
                                     const float *obstacle_capsules /* device [C][8] */, int32_t C, float d_act, float dt,
                                     int32_t substeps, float *qdd_out, float *tau_out, float *stop_out, float *contact_out,
                                     float *contact_lambda, int32_t *contact_pair, uint32_t *status_out, int32_t R,
                                     void *stream);

/* ---- exact flat-capped cylinder obstacles beside the capsules -------------------------------------------------------------------
 * rmp2_dynamics_step_contacts_cylinders is rmp2_dynamics_step_contacts_self -- its argument list, its refusals -- with a table of
 * finite CYLINDERS and a flag: cylinders [Y][8] = (centre xyz, radius, unit axis xyz, half height), fp32, on the device, 16-byte
 * aligned, 0 <= Y <= RMP2_MAX_OBSTACLE_CYLINDERS, shared by the fleet -- the record of RMP2_PRIM_CYLINDER tables, so that the table
 * that steers the robots (rmp2_obstacles) also simulates them.  The axis is used as given: a unit axis is the caller's contract.
 * self_pairs is 0 or 1: with 0 the handle's self pairs are ignored and nothing of them is read.
 * Per frame f with a link capsule (world segment A, A + D, radius r_f) and cylinder y:
 *     (X, Yp, n, sd) = segment_cylinder(record, A, D): the sign of n(s) . D at s = 0 and s = 1 (the distance grows from A on, or the
 *     segment is a point: s = 0; still falling at the far end: s = 1), else 24 halvings of [0, 1] on that sign and one evaluation
 *     at the last midpoint.  X = A + s D is the point on the link's axis, Yp the nearest point of the cylinder's SURFACE, n the
 *     outward unit normal of the surface there, sd the signed distance (X = Yp + sd n), negative where the axis runs inside the
 *     solid; there n is the normal of the nearer of side and cap.  A point on the cylinder's axis takes a fixed perpendicular of the
 *     axis for its radial direction (the cross product with the coordinate axis the cylinder's axis is least aligned with); half
 *     height 0 is a disc.
 *     gap g = sd - r_f;   J[j] = n . (z_j x (X - o_j)) (revolute ancestor dof j; n . z_j prismatic; 0 otherwise);   b = -max(g, 0) / dt.
 * This is NOT the sphere pair at Yp: the normal is the surface's, not (X - Yp) / |X - Yp|, which flips in penetration and is
 * undefined at g = 0.  One row per pair; where the minimum is flat (a link parallel to the side, or lying over a cap) the point is
 * the bisection's choice, and with the slope exactly 0 at s = 0 it is the A end.
 * Cylinder rows compete for the RMP2_MAX_CONTACTS slots by the rule above (g <= d_act, smallest gaps first, ties to the lower pair
 * index, the excess reported as RMP2_CONTACT_OVERFLOW).  The PAIR INDEX of a cylinder row is
 *     RMP2_CONTACT_PAIR_SELF_BASE(F, K, P, C) + F F + f Y + y:
 * the self block of F F values is always reserved, whether or not self pairs are on, and the cylinder pairs follow it, so that a tie
 * goes sphere, plane, capsule, self, cylinder; at most 32 * 2^24 + 512 + 1024 + 1024 + 1024 < 2^31, within int32.  The
 * RMP2_CONTACT_PAIR_CYLINDER_* macros take a cylinder pair apart, RMP2_CONTACT_PAIR_KIND5 tells the five kinds apart.
 * Y == 0 with self_pairs 1 is the self call; Y == 0 with self_pairs 0 the capsules call; and so on down to the stops' step.
 * A non-finite value anywhere in a cylinder record makes every robot NaN.  Beyond the self call's refusals: Y < 0,
 * Y > RMP2_MAX_OBSTACLE_CYLINDERS, a null or misaligned cylinder table with Y > 0, self_pairs outside {0, 1}:
 * RMP2_ERR_INVALID_ARGUMENT.  Robots of at most 9 dofs (RMP2_ERR_UNSUPPORTED beyond).  Stream-ordered, no allocation, no
 * read-back: capturable. */
#define RMP2_MAX_OBSTACLE_CYLINDERS 32
#define RMP2_CONTACT_KIND_CYLINDER 4
#define RMP2_CONTACT_PAIR_CYLINDER_BASE(F, K, P, C) (RMP2_CONTACT_PAIR_SELF_BASE(F, K, P, C) + (int64_t)(F) * (F))
#define RMP2_CONTACT_PAIR_KIND5(pair, F, K, P, C) \
  ((int64_t)(pair) >= RMP2_CONTACT_PAIR_CYLINDER_BASE(F, K, P, C) ? RMP2_CONTACT_KIND_CYLINDER : RMP2_CONTACT_PAIR_KIND4(pair, F, K, P, C))
#define RMP2_CONTACT_PAIR_CYLINDER_FRAME(pair, F, K, P, C, Y) \
  ((int32_t)(((int64_t)(pair) - RMP2_CONTACT_PAIR_CYLINDER_BASE(F, K, P, C)) / (Y)))
#define RMP2_CONTACT_PAIR_CYLINDER_RECORD(pair, F, K, P, C, Y) \
  ((int32_t)(((int64_t)(pair) - RMP2_CONTACT_PAIR_CYLINDER_BASE(F, K, P, C)) % (Y)))
int rmp2_dynamics_step_contacts_cylinders(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive, const float *tau_limit,
                                          const float *q_lower, const float *q_upper, const float *spheres, int32_t K,
                                          const int32_t *csr_offset, const int32_t *csr_index, const float *planes, int32_t P,
                                          const float *obstacle_capsules /* device [C][8] */, int32_t C,
                                          const float *cylinders /* device [Y][8] */, int32_t Y, int32_t self_pairs, float d_act,
                                          float dt, int32_t substeps, float *qdd_out, float *tau_out, float *stop_out,
                                          float *contact_out, float *contact_lambda, int32_t *contact_pair, uint32_t *status_out,
                                          int32_t R, void *stream);

/* ---- per-robot cylinder lists over a shared cylinder pool -----------------------------------------------------------------------
 * rmp2_dynamics_step_contacts_cylinder_lists is rmp2_dynamics_step_contacts_cylinders -- its argument list -- with cylinders [Y][8]
 * a POOL (16-byte aligned, 0 <= Y <= RMP2_MAX_CYLINDER_POOL) and, after Y, every robot's own list over it: cyl_offset (device
 * [R + 1]) and cyl_index (device [cyl_offset[R]]) in the layout of rmp2_obstacles.csr_offset / csr_index.  Robot r's cylinders are
 * cylinders[cyl_index[i]], i in [cyl_offset[r], cyl_offset[r + 1]), in list order, at most RMP2_MAX_CYLINDER_LIST of them: the arrays
 * built for the policy's ragged cylinder mode (RMP2_OBS_RAGGED_SPHERES with RMP2_PRIM_CYLINDER) feed the plant unchanged, with no
 * copy.  The sphere arguments keep both of their forms, independently: the shared table (csr_offset == csr_index == NULL) or lists.
 * Per pair everything is the cylinders call's word for word -- segment_cylinder, the surface's outward normal, g = sd - r_f, the
 * row, b = -max(g, 0) / dt, the cull, the RMP2_MAX_CONTACTS slots and their tie rule, solver, landing, clamps, outputs and status
 * flags; the axis is used as given.  The PAIR INDEX stays RMP2_CONTACT_PAIR_CYLINDER_BASE(F, K, P, C) + f Y + y with Y the POOL's
 * size and y the POOL index, so that the RMP2_CONTACT_PAIR_CYLINDER_* macros decode it unchanged; at most
 * 32 * 2^24 + 512 + 1024 + 1024 + 32 * 2^22 < 2^31, within int32.
 * Contracts, as for the sphere lists: a robot with an empty list gets the results the same call gives it with Y = 0; a robot whose
 * list is strictly ascending gets the results of the cylinders call on the compacted table cylinders[list], pairs mapped through
 * the list (a monotone map keeps the tie order); a robot's results depend on no other robot's list, not on R and not on its lane;
 * an unsorted list gives the same candidate set but possibly another slot order and other bits; a repeated index gives two pairs
 * with identical rows.  On the device, BIT-LEVEL equality is promised among the kernels of this call only -- a robot's bits do not
 * depend on its lane, on the fleet beside it or on where in the pool its records lie; against the cylinders call (other kernels,
 * whose fma contraction is the compiler's) the candidate pairs and the status flags are equal and the floats agree to rounding.
 * INVALID LISTS are refused per robot on the device, by the sphere lists' rule and with their status: a negative start or length,
 * more than RMP2_MAX_CYLINDER_LIST entries, or an entry outside [0, Y) (with Y == 0: any entry).  Every entry is range-checked once
 * per launch, before anything is read through it.  The refused robot's rows are NaN, its contact_pair -1 and its status_out
 * exactly RMP2_CONTACT_LIST_INVALID -- an invalid sphere list and an invalid cylinder list give the same word --, other robots are
 * untouched.  A non-finite value in a cylinder record makes the robots that LIST it NaN, not the fleet.
 * Beyond the cylinders call's refusals, with the pool's cap in place of the table's: cyl_offset or cyl_index NULL with R > 0,
 * Y > RMP2_MAX_CYLINDER_POOL, a null or misaligned pool with Y > 0: RMP2_ERR_INVALID_ARGUMENT.  Robots of at most 9 dofs
 * (RMP2_ERR_UNSUPPORTED beyond).  Stream-ordered, no allocation, no read-back of cyl_offset: capturable. */
#define RMP2_MAX_CYLINDER_LIST 32          /* entries per robot (RMP2_MAX_OBSTACLE_CYLINDERS) */
#define RMP2_MAX_CYLINDER_POOL (1 << 22)   /* records in the pool; 32 * Y must fit the int32 pair index beside the other kinds */
int rmp2_dynamics_step_contacts_cylinder_lists(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive,
                                               const float *tau_limit, const float *q_lower, const float *q_upper,
                                               const float *spheres, int32_t K, const int32_t *csr_offset, const int32_t *csr_index,
                                               const float *planes, int32_t P, const float *obstacle_capsules /* device [C][8] */,
                                               int32_t C, const float *cylinders /* device [Y][8], the pool */, int32_t Y,
                                               const int32_t *cyl_offset /* device [R+1] */,
                                               const int32_t *cyl_index /* device [cyl_offset[R]] */, int32_t self_pairs, float d_act,
                                               float dt, int32_t substeps, float *qdd_out, float *tau_out, float *stop_out,
                                               float *contact_out, float *contact_lambda, int32_t *contact_pair, uint32_t *status_out,
                                               int32_t R, void *stream);

/* The control steps of TWO engines (two robot types of one fleet shard: BASELINE config 5) issued together: arguments as two
 * rmp2_step calls, `stream` shared.  Where a fused instantiation exists for the pair -- a 2-dof and a 3..9-dof robot type,
 * plain steps on shared or ragged sphere tables, both fleets beyond 8 192 robots -- the two steps are ONE grid (the first
 * blocks run A's program, the rest B's; wavefronts stay type-homogeneous); otherwise two launches on `stream`.  Results are
 * those of the two rmp2_step calls either way; rmp2_last_kernel names what ran. */
int rmp2_step_pair(rmp2_handle *ha, const float *qa, const float *qda, const float *goala, int32_t goal_stride_a,
                   const rmp2_obstacles *obsa, const rmp2_outputs *outa, int32_t Ra, rmp2_handle *hb, const float *qb,
                   const float *qdb, const float *goalb, int32_t goal_stride_b, const rmp2_obstacles *obsb,
                   const rmp2_outputs *outb, int32_t Rb, void *stream);

/* Forward kinematics of every frame: T[R][n_frames][16] row-major 4x4
 * (UrdfForwardKinematic.forward, kinematics.py:212-247, for all frames at once).      */
int rmp2_forward_kinematics(rmp2_handle *h, const float *q, float *T, int32_t R, void *stream);

/* Task-map differentiation of the FK map of `frame`
 * (UrdfForwardKinematic.differentiate, kinematics.py:250-270):
 *   x[R][16] = vec(T), xd[R][16] = J qd, J[R][16][n_dof], c[R][16] = Jdot qd.
 * The two differentiate entry points are debug / test entries: they use a per-robot scratch buffer owned by the handle
 * (grown, with a device synchronisation, on the first call at a larger R), so calls on ONE handle must be issued on one
 * stream at a time; rmp2_step / rmp2_rollout / rmp2_forward_kinematics have no such state -- except while a step fence is
 * attached (rmp2_set_step_fence: one issuing thread per handle) and for the cached pair_begin table of EXPLICIT_PAIRS,
 * which is refreshed on the call's stream when the caller's pair layout changes (keep one layout per handle, or one
 * stream). */
int rmp2_differentiate(rmp2_handle *h, const float *q, const float *qd, int32_t frame, float *x, float *xd,
                       float *J, float *c, int32_t R, void *stream);

/* Task-map differentiation of the chain [FK(frame), TaskmapFrom4x4ToEuler] (taskmap.py:57-67 with
 * euler_from_rotation_matrix, kinematics.py:74-96: theta_y = -asin(r20), theta_z = atan2(r10, r00),
 * theta_x = atan2(r21, r22), i.e. R = Rz Ry Rx), used by the reference's tests/test_taskmaps.py:42-44:
 *   x[R][3] = (theta_x, theta_y, theta_z), xd[R][3] = J qd, J[R][3][n_dof], c[R][3] = Jdot qd,
 * analytically: xd = H^-1 w, J = H^-1 J_w, c = H^-1 (alpha - Hdot xd) with w = H(x) xd.  At gimbal lock
 * (|cos theta_y| < 1e-6, where the reference substitutes 1 for the cosine) the outputs are not finite. */
int rmp2_differentiate_euler(rmp2_handle *h, const float *q, const float *qd, int32_t frame, float *x, float *xd,
                             float *J, float *c, int32_t R, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RMP2_H */

"""Engine: one robot type + one RMP set on one MI355X, driven through the C ABI.

PyTorch is used for device memory, streams and (in fleet.py) torch.distributed only; all
arithmetic happens inside librmp2_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native
from . import descriptor as D
from .urdf import MAX_OBSTACLE_CAPSULES   # include/rmp2.h RMP2_MAX_OBSTACLE_CAPSULES: capsules of dynamics_step(contact_obstacle_capsules=)
from .urdf import MAX_OBSTACLE_CYLINDERS  # include/rmp2.h RMP2_MAX_OBSTACLE_CYLINDERS: cylinders of dynamics_step(contact_cylinders=)

MAX_CONTACTS = 8   # include/rmp2.h RMP2_MAX_CONTACTS
MAX_CONTACT_LIST = 256        # include/rmp2.h RMP2_MAX_CONTACT_LIST: entries per robot of dynamics_step(contact_lists=)
MAX_CONTACT_POOL = 1 << 24    # include/rmp2.h RMP2_MAX_CONTACT_POOL: records in its pool
CONTACT_LIST_INVALID = 16     # include/rmp2.h RMP2_CONTACT_LIST_INVALID: status_out of a robot whose list was refused
MAX_CONTACT_PLANES = 8        # include/rmp2.h RMP2_MAX_CONTACT_PLANES: half-spaces of dynamics_step(contact_planes=)
CONTACT_KIND_SPHERE, CONTACT_KIND_PLANE = 0, 1
CONTACT_KIND_CAPSULE = 2
CONTACT_KIND_SELF = 3          # include/rmp2.h RMP2_CONTACT_KIND_SELF: a pair of the robot's own link capsules
MAX_CONTACT_SELF_FRAMES = 22   # include/rmp2.h RMP2_MAX_CONTACT_SELF_FRAMES: distinct partner frames of set_contact_self_pairs
CONTACT_KIND_CYLINDER = 4      # include/rmp2.h RMP2_CONTACT_KIND_CYLINDER: a link capsule against a flat-capped cylinder obstacle
MAX_CYLINDER_LIST = 32         # include/rmp2.h RMP2_MAX_CYLINDER_LIST: entries per robot of dynamics_step(contact_cylinder_lists=)
MAX_CYLINDER_POOL = 1 << 22    # include/rmp2.h RMP2_MAX_CYLINDER_POOL: records in its pool


def contact_pair_split(pair: int, n_frames: int, K: int, P: int, C: int = 0, self_pairs: bool = False, cylinders: int = 0):
    """(kind, frame, record, end) of a contact_pair value of dynamics_step (include/rmp2.h RMP2_CONTACT_PAIR_* macros): kind is
    CONTACT_KIND_SPHERE (record: the sphere's index in the table or pool, end 0), CONTACT_KIND_PLANE (record: the plane, end: 0
    or 1, the capsule's end point) or CONTACT_KIND_CAPSULE (record: the obstacle capsule, end 0).  n_frames: the robot's frame
    count; K, P, C: the call's sphere, plane and obstacle-capsule counts.  None for an empty slot (-1).  self_pairs: the value
    comes from dynamics_step(contact_self=True), whose self rows are (CONTACT_KIND_SELF, link frame, partner frame, 0).
    cylinders: the Y of dynamics_step(contact_cylinders=), whose cylinder rows -- after the self block of n_frames ** 2 values,
    which that call reserves with or without contact_self -- are (CONTACT_KIND_CYLINDER, frame, cylinder, 0)."""
    pair, base = int(pair), int(n_frames) * int(K)
    if pair < 0:
        return None
    cbase = base + 2 * int(n_frames) * int(P)
    sbase = cbase + int(n_frames) * int(C)
    ybase = sbase + int(n_frames) ** 2
    if cylinders and pair >= ybase:
        if pair >= ybase + int(n_frames) * int(cylinders):
            raise ValueError(f"contact pair {pair} is outside the range of {n_frames} frames, {K} spheres, {P} planes, {C} capsules, "
                             f"the self pairs and {cylinders} cylinders")
        return CONTACT_KIND_CYLINDER, (pair - ybase) // int(cylinders), (pair - ybase) % int(cylinders), 0
    if self_pairs and pair >= sbase:
        if pair >= sbase + int(n_frames) ** 2:
            raise ValueError(f"contact pair {pair} is outside the range of {n_frames} frames, {K} spheres, {P} planes, {C} capsules "
                             "and the self pairs")
        return CONTACT_KIND_SELF, (pair - sbase) // int(n_frames), (pair - sbase) % int(n_frames), 0
    if pair >= cbase + int(n_frames) * int(C):
        raise ValueError(f"contact pair {pair} is outside the range of {n_frames} frames, {K} spheres and {P} planes"
                         + (f" and {C} capsules" if C else ""))
    if pair >= cbase:
        return CONTACT_KIND_CAPSULE, (pair - cbase) // C, (pair - cbase) % C, 0
    if pair < base:
        return CONTACT_KIND_SPHERE, pair // K, pair % K, 0
    r = pair - base
    return CONTACT_KIND_PLANE, (r >> 1) // P, (r >> 1) % P, r & 1


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _is_resident(t, device) -> bool:
    """A contiguous fp32 tensor on `device`: usable by the library as it is (no staging copy)."""
    return (isinstance(t, torch.Tensor) and t.device == device and t.dtype == torch.float32 and t.is_contiguous())


def _require_resident(device, **tensors) -> None:
    for name, t in tensors.items():
        if t is not None and not _is_resident(t, device):
            raise ValueError(f"{name} must be a contiguous fp32 tensor on {device}: a staging copy would be made on "
                             "torch's current stream (not ordered against an explicit launch stream) and, for a bound "
                             "launch, later in-place writes to the original would never be seen")


def _hull_arrays(hulls, what: str, entries: str, n: int):
    """(vert_offset, verts, face_offset, planes) of `hulls` -- a urdf hull set or that tuple -- as int32 / float32 arrays of n entries;
    `what` names the feature and `entries` says what the n entries are in the messages."""
    vo, v, fo, p = (hulls.vert_offset, hulls.verts, hulls.face_offset, hulls.planes) if hasattr(hulls, "planes") else hulls
    vo, fo = np.ascontiguousarray(vo, dtype=np.int32), np.ascontiguousarray(fo, dtype=np.int32)
    v, p = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 4)
    if vo.shape != (n + 1,) or fo.shape != (n + 1,):
        raise ValueError(f"{what}: {entries} ({n}), offsets [{n + 1}]")
    if vo[-1] != len(v) or fo[-1] != len(p):
        raise ValueError(f"{what}: the offsets must end at the number of vertices / planes")
    return vo, v, fo, p


class Engine:
    def __init__(self, desc: D.Desc, device: int | torch.device = 0):
        if not torch.cuda.is_available():
            raise _native.Rmp2Error("no HIP device visible; the RMP2 engine has no CPU fallback")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.desc = desc
        self.n_dof = desc.robot.n_dof
        self.n_frames = desc.robot.n_frames
        self._h = C.c_void_p()
        self._lib = _native.lib()
        self._fence_attached = False  # a bound launch attached a completion fence to the handle (bind(done_fence=))
        _native.check(self._lib.rmp2_create(C.byref(desc), self.device.index or 0, C.byref(self._h)))
        self._dist_leaves = D.distance_leaf_indices(desc)
        self._self_counts = None   # self pairs per pair leaf (set_self_collision), None = off
        self._self_key = None      # the self-pair list and geometry the handle holds (set_self_collision / _hulls), None = off
        self._hulls_key = None     # the link hulls the handle holds (set_link_hulls), None = off
        self._inertials_key = None  # the inertial table and gravity the handle holds (set_inertials), None = off
        self._tau_limit = None     # (bytes, device tensor) of the last host tau_limit of dynamics_step: uploaded once per value
        self._q_limits = None      # (bytes, lower, upper) of the last host q_limits of dynamics_step, likewise
        self._empty_index = None   # one int32 on the device: csr_index of dynamics_step(contact_lists=) when every list is empty

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rmp2_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_kernel(self) -> str:
        """Kernel (mapping of robots to lanes) the last step / rollout of this engine launched."""
        return self._lib.rmp2_last_kernel(self._h).decode()

    # ------------------------------------------------------------------------------
    def obstacles(self, *, spheres=None, p_link=None, p_obs=None, pair_counts: Optional[Sequence[int]] = None,
                  csr_offset=None, csr_index=None, dist=None, link_capsules=None, primitive: Optional[str] = None):
        """Build the per-step `rmp2_obstacles` struct from device tensors (kept alive by the result).
        link_capsules [n_distance_leaves, 8] = (a, radius, b, -) per distance leaf, in its frame's coordinates
        (urdf.link_capsules), with a shared table `spheres`: the control point of a pair is the nearest point of the link's
        capsule to the obstacle, formed inside the step (the fused form of closest_points(link_capsules=) + explicit pairs).
        Attached-point leaves (TaskmapRelative4x4 + CollisionAvoidance) take the same two arguments instead of the per-pair arrays
        (p_link = relative_position, p_obs = normal_vec, dist): their Datamanager fields are then formed inside the step from the
        closest points of link capsule and primitive, per control step -- the form that can roll out."""
        o = D.Obstacles()
        keep = []
        if link_capsules is not None:
            if spheres is None or p_link is not None:
                raise ValueError("link_capsules go with a primitive table: obstacles(spheres=..., link_capsules=...[, csr_offset=, csr_index=])")
            link_capsules = _f32(link_capsules, self.device)
            # (one capsule per leaf that consumes per-pair obstacle data -- distance leaves and attached-point leaves -- in leaf order)
            n_dist = len(D.distance_leaf_indices(self.desc))
            if tuple(link_capsules.shape) != (n_dist, 8):
                raise ValueError(f"link_capsules must be [{n_dist}, 8] (one capsule per distance / attached-point leaf, in leaf order)")
            o.link_capsules = link_capsules.data_ptr()
            keep.append(link_capsules)
        if p_link is not None:
            p_link, p_obs = _f32(p_link, self.device), _f32(p_obs, self.device)
            if p_link.shape != p_obs.shape or p_link.dim() != 3 or p_link.shape[2] != 3:
                raise ValueError("p_link / p_obs must both be [R, P, 3]")
            o.mode, o.n_pairs = D.OBS_EXPLICIT_PAIRS, p_link.shape[1]
            dl = self._dist_leaves
            if pair_counts is None:
                if not dl or o.n_pairs % len(dl):
                    raise ValueError("pair_counts required: pairs do not split evenly over the distance leaves")
                pair_counts = [o.n_pairs // len(dl)] * len(dl)
            if len(pair_counts) != len(dl) or sum(pair_counts) != o.n_pairs:
                raise ValueError("pair_counts must have one entry per distance leaf and sum to P")
            acc, k = 0, 0
            for i in range(self.desc.n_leaves + 1):
                o.pair_begin[i] = acc
                if i < self.desc.n_leaves and i in dl:
                    acc += int(pair_counts[k])
                    k += 1
            o.p_link, o.p_obs = p_link.data_ptr(), p_obs.data_ptr()
            keep += [p_link, p_obs]
            if dist is not None:   # attached-point leaves: p_link = relative_position, p_obs = normal_vec
                dist = _f32(dist, self.device)
                if tuple(dist.shape) != tuple(p_link.shape[:2]):
                    raise ValueError("dist must be [R, P]")
                o.dist = dist.data_ptr()
                keep.append(dist)
        elif spheres is not None:
            spheres = _f32(spheres, self.device)
            if spheres.dim() != 2 or spheres.shape[1] not in (4, 8):
                raise ValueError("spheres must be [K, 4] = (cx, cy, cz, radius) or, for capsules, "
                                 "[K, 8] = (ax, ay, az, radius, bx, by, bz, unused)")
            # 8-float records are capsules (a, radius, b, -) unless primitive="cylinder": (centre, radius, unit axis, half height),
            # the reference's flat-capped cylinder obstacles (simulation.py:245-261)
            if primitive not in (None, "sphere", "capsule", "cylinder"):
                raise ValueError("primitive must be 'sphere', 'capsule' or 'cylinder'")
            if primitive == "cylinder":
                if spheres.shape[1] != 8:
                    raise ValueError("cylinder records are [K, 8] = (cx, cy, cz, radius, ux, uy, uz, half_height)")
                o.primitive = D.PRIM_CYLINDER
            else:
                if primitive is not None and (primitive == "capsule") != (spheres.shape[1] == 8):
                    raise ValueError(f"primitive={primitive!r} does not go with records of {spheres.shape[1]} floats")
                o.primitive = D.PRIM_CAPSULE if spheres.shape[1] == 8 else D.PRIM_SPHERE
            o.n_spheres, o.spheres = spheres.shape[0], spheres.data_ptr()
            keep.append(spheres)
            if csr_offset is not None:
                csr_offset = csr_offset.to(device=self.device, dtype=torch.int32).contiguous()
                csr_index = csr_index.to(device=self.device, dtype=torch.int32).contiguous()
                if csr_index.numel() == 0:   # every list empty: the C ABI still wants a readable pointer (it cannot see the counts)
                    csr_index = torch.zeros(1, dtype=torch.int32, device=self.device)
                o.mode, o.csr_offset, o.csr_index = D.OBS_RAGGED_SPHERES, csr_offset.data_ptr(), csr_index.data_ptr()
                keep += [csr_offset, csr_index]
            else:
                o.mode = D.OBS_SHARED_SPHERES
        else:
            o.mode = D.OBS_NONE
        o._keep = keep
        return o

    def step(self, q: torch.Tensor, qd: torch.Tensor, goal: Optional[torch.Tensor] = None, obstacles=None,
             out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
             M: Optional[torch.Tensor] = None, f: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """One control step for the R robots in q/qd ([R, n_dof] fp32 device tensors).
        Asynchronous on `stream` (default: torch's current stream).  With an explicit raw `stream` every tensor must
        already be a contiguous fp32 tensor on the engine's device (conversion copies would run on torch's current
        stream, unordered against `stream`)."""
        if stream is not None:
            _require_resident(self.device, q=q, qd=qd, goal=goal)
        if self._fence_attached:
            self._attach_fence(None)
        q, qd = _f32(q, self.device), _f32(qd, self.device)
        if q.dim() != 2 or q.shape[1] != self.n_dof or q.shape != qd.shape:
            raise ValueError(f"q and qd must be [R, {self.n_dof}], got {tuple(q.shape)} / {tuple(qd.shape)}")
        R = q.shape[0]
        goal_ptr, goal_stride = None, 0
        if self.desc.goal_floats:
            if goal is None:
                raise ValueError("this RMP set has goal-bearing leaves: pass goal")
            goal = _f32(goal, self.device)
            if goal.dim() == 1:
                if goal.shape[0] != self.desc.goal_floats:
                    raise ValueError(f"goal must have {self.desc.goal_floats} floats")
            elif tuple(goal.shape) == (R, self.desc.goal_floats):
                goal_stride = self.desc.goal_floats
            else:
                raise ValueError(f"goal must be [{self.desc.goal_floats}] or [R, {self.desc.goal_floats}]")
            goal_ptr = goal.data_ptr()
        if self._dist_leaves and (obstacles is None or obstacles.mode == D.OBS_NONE) and self._self_counts is None:
            raise ValueError("this RMP set has distance leaves: pass obstacles=engine.obstacles(...)")
        if out is None:
            out = torch.empty((R, self.n_dof), dtype=torch.float32, device=self.device)
        elif out.shape != q.shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous fp32 [R, n_dof] tensor")
        o = D.Outputs()
        o.qdd = out.data_ptr()
        if status is not None:
            assert status.dtype in (torch.int32, torch.uint32) and status.numel() == R
            o.status = status.data_ptr()
        if M is not None:
            assert M.dtype == torch.float64 and M.numel() == R * self.n_dof * self.n_dof
            o.M = M.data_ptr()
        if f is not None:
            assert f.dtype == torch.float64 and f.numel() == R * self.n_dof
            o.f = f.data_ptr()
        s = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        obs = obstacles if obstacles is not None else None
        rc = self._lib.rmp2_step(self._h, q.data_ptr(), qd.data_ptr(), goal_ptr, goal_stride,
                                 C.byref(obs) if obs is not None else None, C.byref(o), R, s)
        _native.check(rc, self._h)
        return out

    def bind(self, q: torch.Tensor, qd: torch.Tensor, goal: Optional[torch.Tensor] = None, obstacles=None,
             out: Optional[torch.Tensor] = None, stream=None, done_fence=None):
        """Pre-validate and pre-marshal one step on FIXED device buffers (the usual control loop:
        the simulator writes q/qd in place, the engine writes qdd in place).  Returns
        (launch, out): `launch()` is a bare C-ABI call (~2 us of host time).  The launch reads the caller's buffers
        themselves, so q, qd and goal must be contiguous fp32 tensors on the engine's device (anything else would be
        copied once and the copy, not the caller's buffer, would be read forever after).
        `done_fence` (fleet._Fence): signalled by the launch's own completion (rmp2_set_step_fence) -- what the
        obstacle exchange needs to know before it overwrites the table this launch reads."""
        _require_resident(self.device, q=q, qd=qd, goal=goal if self.desc.goal_floats else None, out=out)
        out = self.step(q, qd, goal, obstacles=obstacles, out=out, stream=stream)  # validates + warms up
        R = q.shape[0]
        goal_ptr, goal_stride = None, 0
        keep = [q, qd, out, obstacles]
        if self.desc.goal_floats:
            goal_stride = 0 if goal.dim() == 1 else self.desc.goal_floats
            goal_ptr = goal.data_ptr()
            keep.append(goal)
        o = D.Outputs()
        o.qdd = out.data_ptr()
        s = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        obs_ref = C.byref(obstacles) if obstacles is not None else None
        out_ref = C.byref(o)
        fn, h, qp, qdp = self._lib.rmp2_step, self._h, q.data_ptr(), qd.data_ptr()
        keep.append(o)
        if done_fence is None:
            def launch(_keep=keep):
                if self._fence_attached:
                    self._attach_fence(None)
                rc = fn(h, qp, qdp, goal_ptr, goal_stride, obs_ref, out_ref, R, s)
                if rc:
                    _native.check(rc, h)
        else:
            keep.append(done_fence)
            setf, fh = self._lib.rmp2_set_step_fence, done_fence._h

            def launch(_keep=keep):
                setf(h, fh)
                self._fence_attached = True
                rc = fn(h, qp, qdp, goal_ptr, goal_stride, obs_ref, out_ref, R, s)
                if rc:
                    _native.check(rc, h)
        return launch, out

    def _attach_fence(self, fence) -> None:
        self._lib.rmp2_set_step_fence(self._h, fence._h if fence is not None else None)
        self._fence_attached = fence is not None

    def obstacle_trajectory(self, tables: torch.Tensor, csr_offset=None, csr_index=None, primitive: Optional[str] = None):
        """Obstacle tables of a rollout with MOVING obstacles: `tables` [n_control_steps, K, 4] (spheres) or
        [n_control_steps, K, 8] (capsules); control step k of rollout(..., obstacles=this) reads tables[k]."""
        tables = _f32(tables, self.device)
        if tables.dim() != 3 or tables.shape[2] not in (4, 8):
            raise ValueError("tables must be [n_control_steps, K, 4] or [n_control_steps, K, 8]")
        o = self.obstacles(spheres=tables[0], csr_offset=csr_offset, csr_index=csr_index, primitive=primitive)
        o.spheres = tables.data_ptr()
        o._keep.append(tables)
        o._table_steps = int(tables.shape[0])
        return o

    def reserve(self, robots: int) -> None:
        """Pre-size the handle's device buffers for steps of up to `robots` robots (rmp2_reserve): afterwards a step never
        allocates -- needed before capturing a stream with a handle whose step is two kernels (solve = "pinv" without an
        inertia leaf, rank-deficient sets); a no-op for every other handle."""
        _native.check(self._lib.rmp2_reserve(self._h, int(robots)), self._h)

    def rollout(self, q: torch.Tensor, qd: torch.Tensor, goal: Optional[torch.Tensor] = None, obstacles=None,
                n_control_steps: int = 1, substeps: int = 10, dt: float = 0.01, out: Optional[torch.Tensor] = None,
                status: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """Closed-loop rollout in ONE launch: `n_control_steps` x (control step, then `substeps` semi-implicit
        Euler ticks of `dt` with qdd held).  q and qd (contiguous fp32 device tensors) are advanced IN PLACE;
        returns the last qdd.  obstacles = obstacle_trajectory(...): the obstacles move between control steps."""
        for t in (q, qd):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("rollout needs contiguous fp32 CUDA tensors (they are updated in place)")
        if q.dim() != 2 or q.shape[1] != self.n_dof or q.shape != qd.shape:
            raise ValueError(f"q and qd must be [R, {self.n_dof}]")
        if self._fence_attached:
            self._attach_fence(None)
        R = q.shape[0]
        goal_ptr, goal_stride = None, 0
        if self.desc.goal_floats:
            if goal is None:
                raise ValueError("this RMP set has goal-bearing leaves: pass goal")
            goal = _f32(goal, self.device)
            goal_stride = 0 if goal.dim() == 1 else self.desc.goal_floats
            goal_ptr = goal.data_ptr()
        if self._dist_leaves and (obstacles is None or obstacles.mode == D.OBS_NONE):
            raise ValueError("this RMP set has distance leaves: pass obstacles=engine.obstacles(...)")
        if out is None:
            out = torch.empty((R, self.n_dof), dtype=torch.float32, device=self.device)
        elif not _is_resident(out, self.device) or tuple(out.shape) != (R, self.n_dof):
            raise ValueError("out must be a contiguous fp32 [R, n_dof] tensor on the engine's device")
        o = D.Outputs()
        o.qdd = out.data_ptr()
        if status is not None:
            if not (isinstance(status, torch.Tensor) and status.device == self.device and status.is_contiguous()
                    and status.dtype in (torch.int32, torch.uint32) and status.numel() == R):
                raise ValueError("status must be a contiguous int32 / uint32 tensor of R elements on the engine's device")
            o.status = status.data_ptr()
        table_steps = int(getattr(obstacles, "_table_steps", 0)) if obstacles is not None else 0
        if table_steps > 1 and table_steps != int(n_control_steps):
            raise ValueError(f"the obstacle trajectory holds {table_steps} tables, the rollout has {n_control_steps} control steps")
        cfg = D.RolloutCfg(int(n_control_steps), int(substeps), float(dt), table_steps)
        s = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.rmp2_rollout(self._h, q.data_ptr(), qd.data_ptr(), goal_ptr, goal_stride,
                                    C.byref(obstacles) if obstacles is not None else None, C.byref(cfg), C.byref(o), R, s)
        _native.check(rc, self._h)
        # q and qd were advanced through their raw pointers: tell torch (version counters; an in-place operation on an empty
        # slice launches nothing) -- RmpCore's fused route after update_distances relies on "same q, unmodified"
        q[:0].zero_()
        qd[:0].zero_()
        return out

    def forward_kinematics(self, q: torch.Tensor) -> torch.Tensor:
        q = _f32(q, self.device)
        R = q.shape[0]
        T = torch.empty((R, self.n_frames, 4, 4), dtype=torch.float32, device=self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        _native.check(self._lib.rmp2_forward_kinematics(self._h, q.data_ptr(), T.data_ptr(), R, s), self._h)
        return T

    def closest_points(self, q: torch.Tensor, table, link_capsules=None):
        """Closest-point preprocessing stage on its own (simulation.py:462-484 calculate_distances):
        returns (p_link, p_obs), each [R, n_distance_leaves * K, 3], for the shared primitive `table`
        built by obstacles(spheres=...).  The pair arrays can be fed back as obstacles(p_link=, p_obs=).
        link_capsules [n_distance_leaves, 8] = (a, radius, b, -) in each leaf's frame coordinates: the control point of a
        pair is then the nearest point of the LINK's capsule to the obstacle (different per pair, as PyBullet reports it),
        not the frame origin."""
        q = _f32(q, self.device)
        R = q.shape[0]
        n_dist = sum(1 for i in range(self.desc.n_leaves) if self.desc.leaves[i].taskmap == D.TASKMAP_FK_DISTANCE)
        P = n_dist * int(table.n_spheres)
        p_link = torch.empty((R, P, 3), dtype=torch.float32, device=self.device)
        p_obs = torch.empty_like(p_link)
        s = torch.cuda.current_stream(self.device).cuda_stream
        lc_ptr = None
        if link_capsules is not None:
            link_capsules = _f32(link_capsules, self.device)
            if tuple(link_capsules.shape) != (n_dist, 8):
                raise ValueError(f"link_capsules must be [{n_dist}, 8] (one capsule per distance leaf, in leaf order)")
            lc_ptr = link_capsules.data_ptr()
        _native.check(self._lib.rmp2_closest_points_links(self._h, q.data_ptr(), C.byref(table), lc_ptr, p_link.data_ptr(),
                                                          p_obs.data_ptr(), R, s), self._h)
        return p_link, p_obs

    def set_link_hulls(self, hulls) -> None:
        """Convex-hull link geometry (include/rmp2.h rmp2_set_link_hulls): `hulls` = urdf.link_hulls(...) (one hull per distance /
        attached-point leaf, leaf order, in each leaf's frame coordinates) or a tuple (vert_offset, verts, face_offset, planes).
        Every later step with a shared sphere / capsule table forms each pair from the leaf's hull (the hull stage, then the
        explicit-pair step).  None turns it off."""
        if hulls is None:
            if self._hulls_key is not None:
                _native.check(self._lib.rmp2_set_link_hulls(self._h, 0, None, None, None, None), self._h)
            self._hulls_key = None
            return
        n = len(self._dist_leaves)
        vo, v, fo, p = _hull_arrays(hulls, "link hulls", "one hull per distance / attached-point leaf", n)
        key = (vo.tobytes(), v.tobytes(), fo.tobytes(), p.tobytes())
        if key == self._hulls_key:
            return   # (the same hulls: nothing to upload)
        _native.check(self._lib.rmp2_set_link_hulls(self._h, n, vo.ctypes.data, v.ctypes.data, fo.ctypes.data, p.ctypes.data), self._h)
        self._hulls_key = key

    @property
    def has_link_hulls(self) -> bool:
        return self._hulls_key is not None

    def closest_points_hulls(self, q: torch.Tensor, table):
        """The hull stage on its own (rmp2_closest_points_hulls) for the shared table built by obstacles(spheres=...):
        (p_link, p_obs, dist) [R, L K, 3], [R, L K, 3], [R, L K]; pair leaf i owns pairs [i K, (i + 1) K).  Distance leaves: the
        nearest points of hull and primitive in the base frame; attached-point leaves: relative_position, normal_vec, distance."""
        if self._hulls_key is None:
            raise ValueError("link hulls are off: set_link_hulls first")
        q = _f32(q, self.device)
        R, P = q.shape[0], len(self._dist_leaves) * int(table.n_spheres)
        p_link = torch.empty((R, P, 3), dtype=torch.float32, device=self.device)
        p_obs = torch.empty_like(p_link)
        dist = torch.empty((R, P), dtype=torch.float32, device=self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        _native.check(self._lib.rmp2_closest_points_hulls(self._h, q.data_ptr(), C.byref(table), p_link.data_ptr(), p_obs.data_ptr(),
                                                          dist.data_ptr(), R, s), self._h)
        return p_link, p_obs, dist

    def set_self_collision(self, pairs, capsules) -> None:
        """Self collision (include/rmp2.h rmp2_set_self_collision): `pairs` = [(leaf ordinal, frame B or -1)] as
        urdf.self_collision_pairs returns them (ordinal i = the i-th distance / attached-point leaf in leaf order), `capsules`
        [n_frames + 1, 8] = urdf.self_collision_capsules.  Every later step forms the self pairs on the device and appends them
        to each leaf's obstacle pairs (obstacle input NONE or a shared sphere / capsule table).  Empty `pairs` turns it off."""
        pairs = [(int(a), int(b)) for a, b in (pairs or [])]
        if not pairs:
            if self._self_counts is not None:
                _native.check(self._lib.rmp2_set_self_collision(self._h, 0, None, None), self._h)
            self._self_counts, self._self_key = None, None
            return
        arr, counts = self._self_rows(pairs)
        caps = np.ascontiguousarray(capsules, dtype=np.float32)
        if caps.shape != (self.n_frames + 1, 8):
            raise ValueError(f"capsules must be [{self.n_frames + 1}, 8] (one per frame, then the base link)")
        key = (tuple(pairs), caps.tobytes())
        if self._self_counts is not None and self._self_key == key:
            return   # (the same list: nothing to upload)
        _native.check(self._lib.rmp2_set_self_collision(self._h, len(pairs), arr.ctypes.data, caps.ctypes.data), self._h)
        self._self_counts, self._self_key = counts, key

    def set_self_collision_hulls(self, pairs, hulls) -> None:
        """Self collision on the links' convex hulls (include/rmp2.h rmp2_set_self_collision_hulls): `pairs` as for
        set_self_collision, `hulls` = urdf.self_collision_hulls(...) (n_frames + 1 entries: frame f's link in frame coordinates,
        then the base link).  Every later step forms the self pairs hull against hull and the obstacle pairs of a shared sphere /
        capsule table on the same leaf hulls.  Empty `pairs` turns self collision off (either geometry)."""
        pairs = [(int(a), int(b)) for a, b in (pairs or [])]
        if not pairs:
            self.set_self_collision([], None)
            return
        arr, counts = self._self_rows(pairs)
        n = self.n_frames + 1
        vo, v, fo, p = _hull_arrays(hulls, "hull self pairs", "one hull entry per frame and the base", n)
        key = ("hulls", tuple(pairs), vo.tobytes(), v.tobytes(), fo.tobytes(), p.tobytes())
        if self._self_counts is not None and self._self_key == key:
            return   # (the same list: nothing to upload)
        _native.check(self._lib.rmp2_set_self_collision_hulls(self._h, len(pairs), arr.ctypes.data, n, vo.ctypes.data, v.ctypes.data,
                                                              fo.ctypes.data, p.ctypes.data), self._h)
        self._self_counts, self._self_key = counts, key

    def _self_rows(self, pairs):
        """The (leaf ordinal, frame B) list of the self-collision setters as the library's int32 (leaf, B) rows, and the pairs per
        leaf ordinal (the library keeps each leaf's pairs in the order given, leaves in leaf order)."""
        dl = self._dist_leaves
        if any(not 0 <= a < len(dl) for a, _ in pairs):
            raise ValueError(f"leaf ordinals must lie in [0, {len(dl)})")
        counts = [0] * len(dl)
        for a, _ in pairs:
            counts[a] += 1
        return np.ascontiguousarray([(dl[a], b) for a, b in pairs], dtype=np.int32), counts

    @property
    def has_self_hulls(self) -> bool:
        """True while the self pairs are on hulls (set_self_collision_hulls)."""
        return self._self_counts is not None and self._self_key is not None and self._self_key[0] == "hulls"

    @property
    def self_counts(self):
        """Self pairs per distance / attached-point leaf (leaf order), or None when self collision is off."""
        return None if self._self_counts is None else list(self._self_counts)

    def self_pairs(self, q: torch.Tensor):
        """The self-pair stage on its own (rmp2_self_pairs): (p_link, p_obs, dist) [R, S, 3], [R, S, 3], [R, S]; leaf ordinal
        i's pairs at [S_0 + ... + S_{i-1}, + S_i).  Distance leaves: the nearest points of the two capsule surfaces -- of the
        two hulls after set_self_collision_hulls -- (dist = their distance); attached-point leaves: relative_position in the joint
        frame, normal_vec and distance."""
        if self._self_counts is None:
            raise ValueError("self collision is off: set_self_collision first")
        q = _f32(q, self.device)
        R, S = q.shape[0], sum(self._self_counts)
        p_link = torch.empty((R, S, 3), dtype=torch.float32, device=self.device)
        p_obs = torch.empty_like(p_link)
        dist = torch.empty((R, S), dtype=torch.float32, device=self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        _native.check(self._lib.rmp2_self_pairs(self._h, q.data_ptr(), p_link.data_ptr(), p_obs.data_ptr(), dist.data_ptr(), R, s),
                      self._h)
        return p_link, p_obs, dist

    def set_inertials(self, table, gravity=(0.0, 0.0, -9.81)) -> None:
        """Inverse dynamics' rigid-body model (include/rmp2.h rmp2_set_inertials): `table` [n_frames, 10] = urdf.inertial_table
        (frame f's child link in frame coordinates: m, centre of mass, tensor about it), `gravity` in the base frame.  None turns
        the feature off.  The same table and gravity again upload nothing."""
        if table is None:
            if self._inertials_key is not None:
                _native.check(self._lib.rmp2_set_inertials(self._h, 0, None, None), self._h)
            self._inertials_key = None
            return
        t = np.ascontiguousarray(table.detach().cpu() if isinstance(table, torch.Tensor) else table, dtype=np.float32)
        g = np.ascontiguousarray(gravity, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != 10:
            raise ValueError(f"inertials must be [n_frames, 10], got {list(t.shape)}")
        if g.shape != (3,):
            raise ValueError(f"gravity must have 3 entries, got {list(g.shape)}")
        key = (t.tobytes(), g.tobytes())
        if key == self._inertials_key:
            return   # (the same table: nothing to upload)
        _native.check(self._lib.rmp2_set_inertials(self._h, t.shape[0], t.ctypes.data, g.ctypes.data), self._h)
        self._inertials_key = key

    @property
    def has_inertials(self) -> bool:
        return self._inertials_key is not None

    def set_contact_capsules(self, capsules) -> None:
        """Link capsules for the contacts of dynamics_step(contacts=): host [n_frames, 8] = (a, radius, b, 0) per frame in frame
        coordinates, a zero row where a frame has no capsule (urdf.contact_capsules builds them); None switches them off
        (include/rmp2.h rmp2_set_contact_capsules).  Synchronous."""
        if capsules is None:
            _native.check(self._lib.rmp2_set_contact_capsules(self._h, 0, None), self._h)
            return
        c = np.ascontiguousarray(capsules.detach().cpu() if isinstance(capsules, torch.Tensor) else capsules, dtype=np.float32)
        if c.ndim != 2 or c.shape[1] != 8:
            raise ValueError(f"capsules must be [n_frames, 8], got {list(c.shape)}")
        _native.check(self._lib.rmp2_set_contact_capsules(self._h, c.shape[0], c.ctypes.data), self._h)
        if self._empty_index is None:   # (here, not in the step: dynamics_step allocates nothing and can be captured)
            self._empty_index = torch.zeros(1, dtype=torch.int32, device=self.device)

    def set_contact_self_pairs(self, pairs) -> None:
        """Self contacts of dynamics_step(contact_self=True): host pairs [n, 2] of frames whose link capsules (set_contact_capsules)
        may touch each other (urdf.contact_self_pairs builds them); None or an empty list switches them off (include/rmp2.h
        rmp2_set_contact_self_pairs, which states what is refused).  Synchronous; in any order against set_contact_capsules."""
        p = np.zeros((0, 2), np.int32) if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        _native.check(self._lib.rmp2_set_contact_self_pairs(self._h, len(p), p.ctypes.data if len(p) else None), self._h)

    def inverse_dynamics(self, q: torch.Tensor, qd: torch.Tensor, qdd: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Joint torques tau [R, n] = M(q) qdd + C(q, qd) qd + G(q) (include/rmp2.h rmp2_inverse_dynamics) on the current stream;
        q, qd, qdd [R, n] on the engine's device.  Needs set_inertials."""
        q, qd, qdd = _f32(q, self.device), _f32(qd, self.device), _f32(qdd, self.device)
        if q.dim() != 2 or q.shape[1] != self.n_dof or qd.shape != q.shape or qdd.shape != q.shape:
            raise ValueError(f"q, qd, qdd must all be [R, {self.n_dof}], got {list(q.shape)}, {list(qd.shape)}, {list(qdd.shape)}")
        R = q.shape[0]
        if out is None:
            out = torch.empty((R, self.n_dof), dtype=torch.float32, device=self.device)
        else:
            _require_resident(self.device, out=out)
            if tuple(out.shape) != (R, self.n_dof):
                raise ValueError(f"out must be [{R}, {self.n_dof}]")
        s = torch.cuda.current_stream(self.device).cuda_stream
        _native.check(self._lib.rmp2_inverse_dynamics(self._h, q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), out.data_ptr(), R, s),
                      self._h)
        return out

    def _dynamics_rows(self, names: str, *rows):
        rows = tuple(_f32(x, self.device) for x in rows)
        q = rows[0]
        if q.dim() != 2 or q.shape[1] != self.n_dof or any(x.shape != q.shape for x in rows[1:]):
            raise ValueError(f"{names} must all be [R, {self.n_dof}], got " + ", ".join(str(list(x.shape)) for x in rows))
        return rows

    def _dynamics_out(self, name: str, out, shape):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        _require_resident(self.device, **{name: out})
        if tuple(out.shape) != tuple(shape):
            raise ValueError(f"{name} must be {list(shape)}")
        return out

    def mass_matrix(self, q: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Joint-space mass matrix M(q) [R, n, n] (include/rmp2.h rmp2_mass_matrix: symmetric, both triangles) on the current
        stream; q [R, n] on the engine's device.  Needs set_inertials."""
        (q,) = self._dynamics_rows("q", q)
        R = q.shape[0]
        out = self._dynamics_out("out", out, (R, self.n_dof, self.n_dof))
        s = torch.cuda.current_stream(self.device).cuda_stream
        _native.check(self._lib.rmp2_mass_matrix(self._h, q.data_ptr(), out.data_ptr(), R, s), self._h)
        return out

    def forward_dynamics(self, q: torch.Tensor, qd: torch.Tensor, tau: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Accelerations qdd [R, n] = M(q)^-1 (tau - C(q, qd) qd - G(q)) (include/rmp2.h rmp2_forward_dynamics) on the current
        stream; q, qd, tau [R, n] on the engine's device.  Needs set_inertials."""
        q, qd, tau = self._dynamics_rows("q, qd, tau", q, qd, tau)
        R = q.shape[0]
        out = self._dynamics_out("out", out, (R, self.n_dof))
        s = torch.cuda.current_stream(self.device).cuda_stream
        _native.check(self._lib.rmp2_forward_dynamics(self._h, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), out.data_ptr(), R, s),
                      self._h)
        return out

    def _tau_limit_device(self, tau_limit):
        if tau_limit is None:
            return None
        if isinstance(tau_limit, torch.Tensor) and tau_limit.is_cuda:
            _require_resident(self.device, tau_limit=tau_limit)
            if tuple(tau_limit.shape) != (self.n_dof,):
                raise ValueError(f"tau_limit must be [{self.n_dof}], got {list(tau_limit.shape)}")
            return tau_limit
        t = np.ascontiguousarray(tau_limit.detach().cpu() if isinstance(tau_limit, torch.Tensor) else tau_limit, dtype=np.float32)
        if t.shape != (self.n_dof,):
            raise ValueError(f"tau_limit must be [{self.n_dof}], got {list(t.shape)}")
        if not (t >= 0).all():   # (false for a NaN as well; +inf = no limit on that joint)
            raise ValueError("tau_limit must be >= 0 (inf where a joint has no limit)")
        key = t.tobytes()
        if self._tau_limit is None or self._tau_limit[0] != key:   # (the same values again upload nothing)
            self._tau_limit = (key, torch.from_numpy(t).to(self.device))
        return self._tau_limit[1]

    def _q_limits_device(self, q_limits):
        try:
            lower, upper = q_limits
        except (TypeError, ValueError):
            raise ValueError("q_limits must be a pair (lower, upper)") from None
        on_device = [isinstance(x, torch.Tensor) and x.is_cuda for x in (lower, upper)]
        if all(on_device):
            _require_resident(self.device, q_lower=lower, q_upper=upper)
            for name, x in (("lower", lower), ("upper", upper)):
                if tuple(x.shape) != (self.n_dof,):
                    raise ValueError(f"q_limits {name} must be [{self.n_dof}], got {list(x.shape)}")
            return lower, upper
        if any(on_device):
            raise ValueError("q_limits: lower and upper must both be host arrays or both be device tensors")
        lo, hi = (np.ascontiguousarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32) for x in (lower, upper))
        for name, x in (("lower", lo), ("upper", hi)):
            if x.shape != (self.n_dof,):
                raise ValueError(f"q_limits {name} must be [{self.n_dof}], got {list(x.shape)}")
        if not (lo <= hi).all():   # (false for a NaN as well; -inf / +inf = no limit on that side)
            raise ValueError("q_limits must have lower <= upper and no NaN (-inf / +inf where a joint has no limit)")
        key = lo.tobytes() + hi.tobytes()
        if self._q_limits is None or self._q_limits[0] != key:   # (the same values again upload nothing)
            self._q_limits = (key, torch.from_numpy(lo).to(self.device), torch.from_numpy(hi).to(self.device))
        return self._q_limits[1], self._q_limits[2]

    def dynamics_step(self, q: torch.Tensor, qd: torch.Tensor, u: torch.Tensor, dt: float, substeps: int = 1, drive: str = "accel",
                      tau_limit=None, qdd_out: Optional[torch.Tensor] = None, tau_out: Optional[torch.Tensor] = None,
                      q_limits=None, stop_out: Optional[torch.Tensor] = None, status_out: Optional[torch.Tensor] = None,
                      contacts: Optional[torch.Tensor] = None, d_act: float = 0.0, contact_out: Optional[torch.Tensor] = None,
                      contact_lambda_out: Optional[torch.Tensor] = None, contact_pair_out: Optional[torch.Tensor] = None,
                      contact_lists=None, contact_planes: Optional[torch.Tensor] = None,
                      contact_obstacle_capsules: Optional[torch.Tensor] = None, contact_self: bool = False,
                      contact_cylinders: Optional[torch.Tensor] = None, contact_cylinder_lists=None) -> None:
        """The plant's step (include/rmp2.h rmp2_dynamics_step) on the current stream, IN PLACE on q and qd [R, n] (contiguous
        fp32 on the engine's device): `substeps` times qdd = forward dynamics; qd += dt qdd; q += dt qd.  drive="accel": u is the
        policy's qdd_des and the applied torque is the inverse dynamics of it at every substep's state, clamped by tau_limit;
        drive="torque": u is the torque, held and clamped.  tau_limit: [n] host array (uploaded once per value) or device tensor,
        or None.  qdd_out / tau_out [R, n]: the last substep's qdd and applied torque.  Needs set_inertials.
        q_limits = (lower, upper), [n] host arrays (validated, uploaded once per value) or device tensors: the step with
        inelastic joint-limit stops (include/rmp2.h rmp2_dynamics_step_stops; urdf.read_joint_limits reads them).  stop_out
        [R, n] fp32: the stops' torque of the last substep; status_out [R] int32: RMP2_STOP_ACTIVE (1) / RMP2_STOP_CAPPED (2) over
        the substeps, the largest iteration count in bits 8 and up.  Both need q_limits.  None takes the call without stops.
        contacts = spheres [K, 4] fp32 on the engine's device (K <= 256; the static table the links must stay out of): the step
        with stops AND frictionless inelastic contacts of the link capsules (include/rmp2.h rmp2_dynamics_step_contacts; needs
        set_contact_capsules; q_limits optional).  d_act: metres, the gap up to which a pair is a candidate.  contact_out [R, n]
        fp32: the contacts' joint torque; contact_lambda_out [R, 8] fp32: normal forces; contact_pair_out [R, 8] int32: frame * K
        + sphere, -1 in empty slots; status_out also carries RMP2_CONTACT_ACTIVE (4) / RMP2_CONTACT_OVERFLOW (8).  Without
        contacts= the call takes the paths above.
        contact_lists = (csr_offset [R + 1], csr_index) int32 on the engine's device, with contacts = a POOL [K, 4] (K up to
        MAX_CONTACT_POOL): every robot's own spheres, robot r's being contacts[csr_index[csr_offset[r]:csr_offset[r + 1]]] (at most
        MAX_CONTACT_LIST of them) -- the arrays of obstacles(spheres=, csr_offset=, csr_index=) feed the plant unchanged
        (include/rmp2.h rmp2_dynamics_step_contacts_lists).  contact_pair_out stays frame * K + the POOL index.  The lists are
        checked on the device: a robot with an invalid list (an entry outside [0, K), more than MAX_CONTACT_LIST entries, a
        negative length) gets NaN rows and status_out == CONTACT_LIST_INVALID; nothing is read back, the call stays capturable.
        contact_planes = half-spaces [P, 4] fp32 = (unit normal, d) on the engine's device (P <= MAX_CONTACT_PLANES; free space
        n . x >= d; urdf.contact_planes / urdf.floor build them): a floor or walls beside the spheres, with or without contacts=
        and contact_lists= (include/rmp2.h rmp2_dynamics_step_contacts_planes; needs set_contact_capsules).  Every capsule gives
        two rows per plane, one per end point; contact_pair_out holds n_frames * K + 2 * (frame * P + plane) + end for them
        (contact_pair_split takes a value apart).  Without contact_planes= the call takes the routes above, unchanged.
        contact_obstacle_capsules = capsule obstacles [C, 8] fp32 = (a, radius, b, 0) on the engine's device (C <=
        MAX_OBSTACLE_CAPSULES; urdf.capsule_obstacles / urdf.cylinders_as_capsules build them): posts and bars shared by the fleet,
        with or without contacts=, contact_lists= and contact_planes= (include/rmp2.h rmp2_dynamics_step_contacts_capsules; needs
        set_contact_capsules, which sets the LINK capsules).  One row per link capsule and obstacle, at the nearest points of the
        two axes; contact_pair_out holds n_frames * (K + 2 P) + frame * C + capsule for them.  Without it the call takes the
        routes above, unchanged.
        contact_self=True: the robot's own link capsules against each other, the pairs of set_contact_self_pairs, with or without
        any of the obstacle arguments (include/rmp2.h rmp2_dynamics_step_contacts_self; needs set_contact_capsules).  One row per
        pair; contact_pair_out holds n_frames * (K + 2 P + C) + link * n_frames + partner for them (contact_pair_split(...,
        self_pairs=True)).  With no pairs set it is the call without the flag.
        contact_cylinders = flat-capped cylinder obstacles [Y, 8] fp32 = (centre, radius, unit axis, half height) on the engine's
        device (Y <= MAX_OBSTACLE_CYLINDERS; urdf.cylinder_obstacles builds them from configs.cylinder_record rows): the
        reference's posts as what they are, exact flat caps and rims, shared by the fleet, with or without any of the arguments
        above (include/rmp2.h rmp2_dynamics_step_contacts_cylinders; needs set_contact_capsules).  It is the table that
        obstacles(..., primitive="cylinder") hands to the policy.  One row per link capsule and cylinder, at the point of the link's
        axis nearest the cylinder, along the outward normal of the cylinder's surface; contact_pair_out holds n_frames * (K + 2 P +
        C) + n_frames ** 2 + frame * Y + cylinder for them (contact_pair_split(..., cylinders=Y)).  contact_self says whether the
        handle's self pairs take part.  Without it the call takes the routes above, unchanged.
        contact_cylinder_lists = (cyl_offset [R + 1], cyl_index) int32 on the engine's device, with contact_cylinders = a POOL [Y, 8]
        (Y up to MAX_CYLINDER_POOL): every robot's own cylinders, robot r's being contact_cylinders[cyl_index[cyl_offset[r]:
        cyl_offset[r + 1]]] (at most MAX_CYLINDER_LIST of them; urdf.cylinder_scenes builds the three arrays) -- the arrays of
        obstacles(spheres=pool, csr_offset=, csr_index=, primitive="cylinder") feed the plant unchanged (include/rmp2.h
        rmp2_dynamics_step_contacts_cylinder_lists).  contacts= / contact_lists= keep both of their forms beside it.
        contact_pair_out stays ... + frame * Y + the POOL index (contact_pair_split(..., cylinders=Y)).  The lists are checked on the
        device like contact_lists: a robot with an invalid list gets NaN rows and status_out == CONTACT_LIST_INVALID, a robot that
        lists a non-finite record NaN rows; nothing is read back, the call stays capturable.  Without it every route is the one
        above."""
        _require_resident(self.device, q=q, qd=qd)
        drives = {"torque": 0, "accel": 1}
        if drive not in drives:
            raise ValueError(f"drive must be 'accel' or 'torque', got {drive!r}")
        q, qd, u = self._dynamics_rows("q, qd, u", q, qd, u)
        R = q.shape[0]
        for name, o in (("qdd_out", qdd_out), ("tau_out", tau_out), ("stop_out", stop_out)):
            if o is not None:
                self._dynamics_out(name, o, (R, self.n_dof))
        lim = self._tau_limit_device(tau_limit)
        s = torch.cuda.current_stream(self.device).cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()

        def check_int(name, t, shape):
            if t is not None and (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.int32
                                  or tuple(t.shape) != tuple(shape) or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous int32 {list(shape)} tensor on {self.device}")

        if contact_cylinder_lists is not None and contact_cylinders is None:
            raise ValueError("contact_cylinder_lists needs contact_cylinders (the pool the lists index)")
        if (contacts is not None or contact_planes is not None or contact_obstacle_capsules is not None or contact_self
                or contact_cylinders is not None):
            P = C = Y = 0
            if contact_cylinders is not None:
                cyl = contact_cylinders
                _require_resident(self.device, contact_cylinders=cyl)
                if cyl.dim() != 2 or cyl.shape[1] != 8 or cyl.dtype != torch.float32 or not cyl.is_contiguous():
                    raise ValueError("contact_cylinders must be a contiguous fp32 [Y, 8] tensor (centre, radius, unit axis, half height), "
                                     f"got {list(cyl.shape)}")
                Y = int(cyl.shape[0])
                if contact_cylinder_lists is not None:
                    if Y > MAX_CYLINDER_POOL:
                        raise ValueError(f"contact_cylinders holds {Y} cylinders, at most {MAX_CYLINDER_POOL} in a pool")
                elif Y > MAX_OBSTACLE_CYLINDERS:
                    raise ValueError(f"contact_cylinders holds {Y} cylinders, at most {MAX_OBSTACLE_CYLINDERS}")
            if contact_obstacle_capsules is not None:
                oc = contact_obstacle_capsules
                _require_resident(self.device, contact_obstacle_capsules=oc)
                if oc.dim() != 2 or oc.shape[1] != 8 or oc.dtype != torch.float32 or not oc.is_contiguous():
                    raise ValueError("contact_obstacle_capsules must be a contiguous fp32 [C, 8] tensor (a, radius, b, 0), got "
                                     f"{list(oc.shape)}")
                C = int(oc.shape[0])
                if C > MAX_OBSTACLE_CAPSULES:
                    raise ValueError(f"contact_obstacle_capsules holds {C} capsules, at most {MAX_OBSTACLE_CAPSULES}")
            if contact_planes is not None:
                _require_resident(self.device, contact_planes=contact_planes)
                if (contact_planes.dim() != 2 or contact_planes.shape[1] != 4 or contact_planes.dtype != torch.float32
                        or not contact_planes.is_contiguous()):
                    raise ValueError(f"contact_planes must be a contiguous fp32 [P, 4] tensor (normal, d), got {list(contact_planes.shape)}")
                P = int(contact_planes.shape[0])
                if P > MAX_CONTACT_PLANES:
                    raise ValueError(f"contact_planes holds {P} planes, at most {MAX_CONTACT_PLANES}")
            if contacts is None and contact_lists is not None:
                raise ValueError("contact_lists needs contacts (the pool the lists index)")
            K = 0
            if contacts is not None:
                _require_resident(self.device, contacts=contacts)
                if contacts.dim() != 2 or contacts.shape[1] != 4:
                    raise ValueError(f"contacts must be [K, 4] spheres (centre, radius), got {list(contacts.shape)}")
                K = int(contacts.shape[0])
            if contact_out is not None:
                self._dynamics_out("contact_out", contact_out, (R, self.n_dof))
            if contact_lambda_out is not None:
                self._dynamics_out("contact_lambda_out", contact_lambda_out, (R, MAX_CONTACTS))
            check_int("contact_pair_out", contact_pair_out, (R, MAX_CONTACTS))
            check_int("status_out", status_out, (R,))
            lower, upper = (None, None) if q_limits is None else self._q_limits_device(q_limits)
            def csr_pair(what, names, pair):
                try:
                    offset, index = pair
                except (TypeError, ValueError):
                    raise ValueError(f"{what} must be a pair ({names[0]}, {names[1]})") from None
                for name, t, shape in ((names[0], offset, (R + 1,)), (names[1], index, None)):
                    if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.int32
                            or not t.is_contiguous() or (t.dim() != 1 if shape is None else tuple(t.shape) != shape)):
                        raise ValueError(f"{what} {name} must be a contiguous int32 {'1-D' if shape is None else list(shape)} "
                                         f"tensor on {self.device}")
                if index.numel() == 0:   # every list empty: the C ABI still wants a readable pointer (it cannot see the counts)
                    index = self._empty_index   # (made by set_contact_capsules; without capsules the call is refused anyway)
                return offset, index

            csr_offset = csr_index = None
            if contact_lists is not None:
                csr_offset, csr_index = csr_pair("contact_lists", ("csr_offset", "csr_index"), contact_lists)
            head = (self._h, q.data_ptr(), qd.data_ptr(), u.data_ptr(), drives[drive], ptr(lim), ptr(lower), ptr(upper),
                    contacts.data_ptr() if K else None, K)
            tail = (float(d_act), float(dt), int(substeps), ptr(qdd_out), ptr(tau_out), ptr(stop_out), ptr(contact_out),
                    ptr(contact_lambda_out), ptr(contact_pair_out), ptr(status_out), R, s)
            lists = (ptr(csr_offset), ptr(csr_index))
            if contact_cylinder_lists is not None:
                cyl_offset, cyl_index = csr_pair("contact_cylinder_lists", ("cyl_offset", "cyl_index"), contact_cylinder_lists)
                rc = self._lib.rmp2_dynamics_step_contacts_cylinder_lists(*head, *lists, contact_planes.data_ptr() if P else None, P,
                                                                          contact_obstacle_capsules.data_ptr() if C else None, C,
                                                                          contact_cylinders.data_ptr() if Y else None, Y,
                                                                          ptr(cyl_offset), ptr(cyl_index), 1 if contact_self else 0,
                                                                          *tail)
            elif contact_cylinders is not None:
                rc = self._lib.rmp2_dynamics_step_contacts_cylinders(*head, *lists, contact_planes.data_ptr() if P else None, P,
                                                                     contact_obstacle_capsules.data_ptr() if C else None, C,
                                                                     contact_cylinders.data_ptr() if Y else None, Y,
                                                                     1 if contact_self else 0, *tail)
            elif contact_self:
                rc = self._lib.rmp2_dynamics_step_contacts_self(*head, *lists, contact_planes.data_ptr() if P else None, P,
                                                                contact_obstacle_capsules.data_ptr() if C else None, C, *tail)
            elif contact_obstacle_capsules is not None:
                rc = self._lib.rmp2_dynamics_step_contacts_capsules(*head, *lists, contact_planes.data_ptr() if P else None, P,
                                                                    contact_obstacle_capsules.data_ptr() if C else None, C, *tail)
            elif contact_planes is not None:
                rc = self._lib.rmp2_dynamics_step_contacts_planes(*head, *lists, contact_planes.data_ptr() if P else None, P, *tail)
            elif contact_lists is not None:
                rc = self._lib.rmp2_dynamics_step_contacts_lists(*head, *lists, *tail)
            else:
                rc = self._lib.rmp2_dynamics_step_contacts(*head, *tail)
            _native.check(rc, self._h)
            return
        if contact_lists is not None:
            raise ValueError("contact_lists needs contacts (the pool the lists index)")
        if contact_out is not None or contact_lambda_out is not None or contact_pair_out is not None:
            raise ValueError("contact_out / contact_lambda_out / contact_pair_out need contacts")
        if q_limits is None:
            if stop_out is not None or status_out is not None:
                raise ValueError("stop_out / status_out need q_limits")
            _native.check(self._lib.rmp2_dynamics_step(self._h, q.data_ptr(), qd.data_ptr(), u.data_ptr(), drives[drive], ptr(lim),
                                                       float(dt), int(substeps), ptr(qdd_out), ptr(tau_out), R, s), self._h)
            return
        if status_out is not None:
            if (not isinstance(status_out, torch.Tensor) or status_out.device != self.device or status_out.dtype != torch.int32
                    or tuple(status_out.shape) != (R,) or not status_out.is_contiguous()):
                raise ValueError(f"status_out must be a contiguous int32 [{R}] tensor on {self.device}")
        lower, upper = self._q_limits_device(q_limits)
        _native.check(self._lib.rmp2_dynamics_step_stops(self._h, q.data_ptr(), qd.data_ptr(), u.data_ptr(), drives[drive], ptr(lim),
                                                         lower.data_ptr(), upper.data_ptr(), float(dt), int(substeps), ptr(qdd_out),
                                                         ptr(tau_out), ptr(stop_out), ptr(status_out), R, s), self._h)

    def differentiate(self, q: torch.Tensor, qd: torch.Tensor, frame: int):
        q, qd = _f32(q, self.device), _f32(qd, self.device)
        R, n = q.shape
        x, xd, c = (torch.empty((R, 16), dtype=torch.float32, device=self.device) for _ in range(3))
        J = torch.empty((R, 16, n), dtype=torch.float32, device=self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        _native.check(self._lib.rmp2_differentiate(self._h, q.data_ptr(), qd.data_ptr(), int(frame), x.data_ptr(),
                                                   xd.data_ptr(), J.data_ptr(), c.data_ptr(), R, s), self._h)
        return x, xd, J, c

    def differentiate_euler(self, q: torch.Tensor, qd: torch.Tensor, frame: int):
        """(x, xd, J, c) of the chain [FK(frame), TaskmapFrom4x4ToEuler]: x, xd, c [R,3], J [R,3,n]."""
        q, qd = _f32(q, self.device), _f32(qd, self.device)
        R, n = q.shape
        x, xd, c = (torch.empty((R, 3), dtype=torch.float32, device=self.device) for _ in range(3))
        J = torch.empty((R, 3, n), dtype=torch.float32, device=self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        _native.check(self._lib.rmp2_differentiate_euler(self._h, q.data_ptr(), qd.data_ptr(), int(frame), x.data_ptr(),
                                                         xd.data_ptr(), J.data_ptr(), c.data_ptr(), R, s), self._h)
        return x, xd, J, c


def bind_pair(eng_a: "Engine", q_a, qd_a, goal_a, obstacles_a, out_a, eng_b: "Engine", q_b, qd_b, goal_b, obstacles_b, out_b,
              stream=None):
    """Pre-marshal the control steps of TWO engines (two robot types of one shard) as one C-ABI call, rmp2_step_pair: one fused
    grid where the library has an instantiation for the pair (include/rmp2.h), two launches otherwise.  Buffers as for
    Engine.bind (contiguous fp32 tensors on the engines' device, read and written in place).  Returns launch()."""
    if eng_a.device != eng_b.device:
        raise ValueError("bind_pair: both engines must live on one device")
    for eng, q, qd, goal, obs, out in ((eng_a, q_a, qd_a, goal_a, obstacles_a, out_a), (eng_b, q_b, qd_b, goal_b, obstacles_b, out_b)):
        _require_resident(eng.device, q=q, qd=qd, goal=goal if eng.desc.goal_floats else None, out=out)
        eng.step(q, qd, goal, obstacles=obs, out=out, stream=stream)   # validates the arguments (and warms the kernels up)
    lib = eng_a._lib
    outs, args = [], []
    for eng, q, qd, goal, obs, out in ((eng_a, q_a, qd_a, goal_a, obstacles_a, out_a), (eng_b, q_b, qd_b, goal_b, obstacles_b, out_b)):
        o = D.Outputs()
        o.qdd = out.data_ptr()
        outs.append(o)
        gp = goal.data_ptr() if eng.desc.goal_floats else None
        gs = 0 if (not eng.desc.goal_floats or goal.dim() == 1) else eng.desc.goal_floats
        args += [eng._h, q.data_ptr(), qd.data_ptr(), gp, gs, C.byref(obs) if obs is not None else None, C.byref(o), q.shape[0]]
    s = stream if stream is not None else torch.cuda.current_stream(eng_a.device).cuda_stream
    keep = (q_a, qd_a, goal_a, obstacles_a, out_a, q_b, qd_b, goal_b, obstacles_b, out_b, outs)
    fn = lib.rmp2_step_pair

    def launch(_keep=keep):
        rc = fn(*args, s)
        if rc:
            _native.check(rc, eng_a._h)
    return launch

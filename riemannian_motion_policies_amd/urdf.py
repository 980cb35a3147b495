"""URDF -> flat kinematic table ("kinematic compiler", host side, setup time only).

This is the setup stage of the hot path: it turns a URDF into the constant tables the
HIP kernels index.  It restates the *semantics* of the reference's setup code

  * helper/urdf_parsing.py:57-97   (find base link, breadth-first attach joints, ids in
                                    creation order)
  * helper/urdf_parsing.py:134-147 (backward paths root -> element, by joint name)
  * kinematics.py:163-209          (frame names, padded chains, q re-ordering, T_constant
                                    from rpy/xyz with R = R_x(roll) @ R_y(pitch) @ R_z(yaw)
                                    -- reference quirk Q7 --, axis, one-hot joint types)

but emits a parent-index tree + depth-first schedule instead of padded chain tables,
because the kernels walk the tree once per robot and never re-multiply a chain.

Nothing here touches the GPU; the table is plain numpy and is serialised into the C
descriptor by `descriptor.py`.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import List, Sequence
from xml.etree import ElementTree

import numpy as np

JOINT_FIXED = 0
JOINT_REVOLUTE = 1
JOINT_PRISMATIC = 2
_TYPE_CODE = {"fixed": JOINT_FIXED, "revolute": JOINT_REVOLUTE, "prismatic": JOINT_PRISMATIC}

_ROBOT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "robots")
PANDA_URDF = os.path.join(_ROBOT_DIR, "panda_kinematics.urdf")
TWO_JOINT_URDF = os.path.join(_ROBOT_DIR, "two_joint_kinematics.urdf")

# PyBullet motor-joint order of the two reference robots (helper/pybullet_helper.py:8-19
# applied to the reference URDFs; SURVEY section 8 header).
PANDA_ORDER = [f"panda_joint{i}" for i in range(1, 8)] + ["panda_finger_joint1", "panda_finger_joint2"]
TWO_JOINT_ORDER = ["joint_1", "joint_2"]


def _floats(text: str | None, n: int = 3) -> List[float]:
    if text is None:
        return [0.0] * n
    vals = [float(t) for t in text.split()]
    if len(vals) != n:
        raise ValueError(f"expected {n} numbers, got {text!r}")
    return vals


def _rot_x(a: np.float32) -> np.ndarray:
    c, s = np.cos(a, dtype=np.float32), np.sin(a, dtype=np.float32)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float32)


def _rot_y(a: np.float32) -> np.ndarray:
    c, s = np.cos(a, dtype=np.float32), np.sin(a, dtype=np.float32)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float32)


def _rot_z(a: np.float32) -> np.ndarray:
    c, s = np.cos(a, dtype=np.float32), np.sin(a, dtype=np.float32)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)


def rotation_from_rpy_reference_order(rpy: Sequence[float]) -> np.ndarray:
    """fp32 R = R_x(roll) @ R_y(pitch) @ R_z(yaw)  (kinematics.py:123-127, quirk Q7).

    The URDF standard is R_z @ R_y @ R_x; the reference multiplies the other way round.
    Both agree whenever at most one angle is non-zero, which holds for every joint of the
    two reference robots.  The reference's order is reproduced on purpose.
    """
    r, p, y = (np.float32(v) for v in rpy)
    return ((_rot_x(r) @ _rot_y(p)).astype(np.float32) @ _rot_z(y)).astype(np.float32)


@dataclass
class _Elem:
    name: str
    link_name: str
    joint_type: str = "fixed"
    rpy: List[float] = field(default_factory=lambda: [0.0, 0.0, 0.0])
    xyz: List[float] = field(default_factory=lambda: [0.0, 0.0, 0.0])
    axis: List[float] = field(default_factory=lambda: [0.0, 0.0, 0.0])
    has_collision: bool = False
    parent: int = -1  # element id of the parent (0 = root element)


@dataclass
class KinematicTable:
    """Constant tables of one robot type.  Frame index = reference frame order."""

    frame_names: List[str]
    parent: np.ndarray  # int32 [F], parent frame index, -1 = child of the base link
    joint_type: np.ndarray  # int32 [F], JOINT_*
    q_index: np.ndarray  # int32 [F], index into the caller's q vector, -1 = not actuated
    axis: np.ndarray  # float32 [F,3], joint axis in the joint frame
    T_const: np.ndarray  # float32 [F,4,4], parent-link -> joint frame at q = 0
    has_collision: np.ndarray  # bool [F]
    order: List[str]  # caller's joint order (names), len = n_dof
    link_names: List[str]
    limits_lower: np.ndarray  # float32 [F] (nan when the joint has no <limit>)
    limits_upper: np.ndarray  # float32 [F]

    @property
    def n_frames(self) -> int:
        return len(self.frame_names)

    @property
    def n_dof(self) -> int:
        return len(self.order)

    def frame_index(self, name: str) -> int:
        try:
            return self.frame_names.index(name)
        except ValueError:
            raise KeyError(f"unknown frame {name!r}; known: {self.frame_names}") from None

    # -- views that mirror the reference's own tables (used by the golden-table test) ----
    def backward_paths(self) -> List[List[str]]:
        """Root -> frame joint-name paths (helper/urdf_parsing.py:134-147)."""
        paths = []
        for i in range(self.n_frames):
            path, j = [], i
            while j >= 0:
                path.insert(0, self.frame_names[j])
                j = int(self.parent[j])
            paths.append(path)
        return paths

    def q_reordering(self) -> List[int]:
        """kinematics.py:197: index into q, or n_dof for "append 0"."""
        return [int(k) if k >= 0 else self.n_dof for k in self.q_index]

    def ancestor_dof_mask(self, frame: int) -> int:
        """Bit j set  <=>  dof j moves `frame` (its joint is the frame or an ancestor)."""
        mask, j = 0, frame
        while j >= 0:
            if self.q_index[j] >= 0 and self.joint_type[j] != JOINT_FIXED:
                mask |= 1 << int(self.q_index[j])
            j = int(self.parent[j])
        return mask

    def depth_first_schedule(self):
        """Visit order + save/restore slots for a one-pass tree walk.

        Returns (order, restore_slot, save_slot, n_slots): frames are visited in `order`
        (depth-first pre-order, children in reference order).  The walker keeps ONE
        running frame state; `restore_slot[k] >= 0` means "before visiting order[k], reload
        the state saved in that slot" (the parent is not the frame visited just before),
        `restore_slot[k] == -2` means "start from the base", -1 means "continue from the
        previous frame".  `save_slot[k] >= 0` means "after visiting, save the state" (the
        frame has a child that is not visited immediately afterwards).
        """
        F = self.n_frames
        children = [[] for _ in range(F)]
        roots = []
        for i in range(F):
            (roots if self.parent[i] < 0 else children[int(self.parent[i])]).append(i)
        order: List[int] = []
        stack = list(reversed(roots))
        while stack:
            i = stack.pop()
            order.append(i)
            stack.extend(reversed(children[i]))
        pos = {f: k for k, f in enumerate(order)}
        restore = [-1] * F
        save = [-1] * F
        free_at: List[int] = []  # per slot: schedule position after which it is free
        slot_of = {}
        for k, f in enumerate(order):
            p = int(self.parent[f])
            if p < 0:
                restore[k] = -2
            elif k > 0 and order[k - 1] == p:
                restore[k] = -1
            else:
                restore[k] = slot_of[p]
            # does f need saving?  yes if some child is not the next frame in the order
            late = [c for c in children[f] if pos[c] != k + 1]
            if late:
                last_use = max(pos[c] for c in late)
                for s, free in enumerate(free_at):
                    if free < k:
                        free_at[s] = last_use
                        slot_of[f] = s
                        break
                else:
                    free_at.append(last_use)
                    slot_of[f] = len(free_at) - 1
                save[k] = slot_of[f]
        return order, restore, save, len(free_at)


def compile_urdf(urdf_filepath: str, order: Sequence[str]) -> KinematicTable:
    """Parse `urdf_filepath` and build the table for joint order `order`.

    Frame order reproduces the reference exactly: breadth-first over links starting at the
    base link, joints taken in document order (helper/urdf_parsing.py:74-97), frames =
    all non-root elements in creation order (kinematics.py:169-171).
    """
    root = ElementTree.parse(urdf_filepath).getroot()
    links = root.findall("link")
    joints = root.findall("joint")
    if not links or not joints:
        raise ValueError(f"{urdf_filepath}: no <link>/<joint> elements")

    child_links = {j.find("child").attrib["link"] for j in joints}
    base = next((l for l in links if l.attrib["name"] not in child_links), None)
    if base is None:
        raise ValueError("URDF has no base link (every link is the child of a joint)")
    link_by_name = {l.attrib["name"]: l for l in links}

    elems: List[_Elem] = [_Elem(name="<ROOT>", link_name=base.attrib["name"])]
    limits: List[tuple] = [(np.nan, np.nan)]
    todo = [0]
    while todo:
        leaf = todo.pop(0)
        for j in joints:
            if j.find("parent").attrib["link"] != elems[leaf].link_name:
                continue
            jtype = j.attrib["type"]
            if jtype not in _TYPE_CODE:
                raise NotImplementedError(
                    f"joint {j.attrib['name']!r}: type {jtype!r} is not supported "
                    "(the reference handles fixed / revolute / prismatic only, kinematics.py:205-209)")
            origin = j.find("origin")
            axis_el = j.find("axis")
            child = link_by_name[j.find("child").attrib["link"]]
            lim = j.find("limit")
            elems.append(_Elem(
                name=j.attrib["name"],
                link_name=child.attrib["name"],
                joint_type=jtype,
                rpy=_floats(origin.attrib.get("rpy") if origin is not None else None),
                xyz=_floats(origin.attrib.get("xyz") if origin is not None else None),
                axis=(_floats(axis_el.attrib.get("xyz")) if (axis_el is not None and jtype != "fixed")
                      else [0.0, 0.0, 0.0]),
                has_collision=child.find("collision") is not None,
                parent=leaf,
            ))
            limits.append((float(lim.attrib["lower"]), float(lim.attrib["upper"]))
                          if lim is not None and "lower" in lim.attrib else (np.nan, np.nan))
            todo.append(len(elems) - 1)

    frames = elems[1:]
    F = len(frames)
    order = list(order)
    names = [e.name for e in frames]
    for o in order:
        if o not in names:
            raise KeyError(f"joint {o!r} from `order` is not in the URDF")
    T_const = np.zeros((F, 4, 4), dtype=np.float32)
    for i, e in enumerate(frames):
        T_const[i, :3, :3] = rotation_from_rpy_reference_order(e.rpy)
        T_const[i, :3, 3] = np.asarray(e.xyz, dtype=np.float32)
        T_const[i, 3, 3] = 1.0
    q_index = np.array([order.index(e.name) if e.name in order else -1 for e in frames], dtype=np.int32)
    jt = np.array([_TYPE_CODE[e.joint_type] for e in frames], dtype=np.int32)
    for i, e in enumerate(frames):
        if jt[i] != JOINT_FIXED and q_index[i] < 0:
            # reference: q' = gather([q, 0], reorder) -> a movable joint missing from `order`
            # is evaluated at q = 0 (kinematics.py:197,218-219); keep that behaviour.
            pass
    return KinematicTable(
        frame_names=names,
        parent=np.array([e.parent - 1 for e in frames], dtype=np.int32),
        joint_type=jt,
        q_index=q_index,
        axis=np.array([e.axis for e in frames], dtype=np.float32).reshape(F, 3),
        T_const=T_const,
        has_collision=np.array([e.has_collision for e in frames], dtype=bool),
        order=order,
        link_names=[e.link_name for e in frames],
        limits_lower=np.array([l[0] for l in limits[1:]], dtype=np.float32),
        limits_upper=np.array([l[1] for l in limits[1:]], dtype=np.float32),
    )


def fitted_link_capsules(urdf_filepath: str) -> dict:
    """{link name: {"a": [3], "b": [3], "r": float}} of capsules fitted to the collision MESHES of a robot whose kinematics-only
    URDF ships here: `<stem>_link_capsules.json` next to `<stem>_kinematics.urdf` (the Panda's: generated from the vertex sets of
    the reference's collision meshes by tests/golden/make_panda_link_capsules.py -- minimum-volume enclosing capsules, so
    distances to the capsule never exceed distances to the mesh); {} when there is no such file."""
    import json
    stem = os.path.basename(urdf_filepath)
    for suffix in ("_kinematics.urdf", ".urdf"):
        if stem.endswith(suffix):
            stem = stem[: -len(suffix)]
            break
    path = os.path.join(os.path.dirname(urdf_filepath), stem + "_link_capsules.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return json.load(f)["links"]


def link_capsules(urdf_filepath: str, table: KinematicTable, frames: Sequence[str], default_radius: float = 0.06,
                  fitted="auto") -> np.ndarray:
    """Link capsules [len(frames), 8] = (a, radius, b, 0) in FRAME coordinates for the closest-point stage with link
    geometry (Engine.closest_points(link_capsules=), include/rmp2.h rmp2_closest_points_links): the link that moves with
    each frame as a capsule.  The reference asks PyBullet for the closest points on the link's collision SHAPE
    (simulation.py:462-484); here that shape is reduced to a capsule:
      * <cylinder length radius>: the cylinder's axis (local z of the collision origin), shortened by the radius at both ends;
      * <box size>: the box's longest edge as the axis, radius = half the larger of the two other edges, shortened likewise;
      * <sphere radius>: a capsule of zero length;
      * <mesh> / no primitive: the capsule FITTED to the link's collision mesh where one ships with the robot (`fitted`:
        "auto" = fitted_link_capsules(urdf_filepath) -- the Panda's --, a dict of the same shape, or None); otherwise the segment
        from the frame origin to the origin of its first child frame (the next joint), radius `default_radius`."""
    root = ElementTree.parse(urdf_filepath).getroot()
    link_by_name = {l.attrib["name"]: l for l in root.findall("link")}
    fitted = fitted_link_capsules(urdf_filepath) if fitted == "auto" else (fitted or {})
    out = np.zeros((len(frames), 8), dtype=np.float32)
    for i, fr in enumerate(frames):
        f = table.frame_index(fr)
        kids = [c for c in range(table.n_frames) if table.parent[c] == f]
        b = table.T_const[kids[0], :3, 3].astype(np.float64) if kids else np.zeros(3)
        out[i] = _link_capsule(link_by_name.get(table.link_names[f]), fitted.get(table.link_names[f]), b, default_radius)
    return out


def _link_capsule(link, cap, fallback_b, default_radius: float) -> np.ndarray:
    """One row of link_capsules: the capsule of `link` (an URDF <link> element or None) in its own coordinates; `cap` is its
    fitted capsule or None, `fallback_b` the end of the fallback segment from the origin."""
    col = link.find("collision") if link is not None else None
    geom = col.find("geometry") if col is not None else None
    origin = col.find("origin") if col is not None else None
    xyz = np.asarray(_floats(origin.attrib.get("xyz") if origin is not None else None), dtype=np.float64)
    Rc = rotation_from_rpy_reference_order(_floats(origin.attrib.get("rpy") if origin is not None else None)).astype(np.float64)
    prim = None
    if geom is not None:
        for tag in ("cylinder", "box", "sphere"):
            if geom.find(tag) is not None:
                prim = (tag, geom.find(tag))
    if prim is not None and prim[0] == "cylinder":
        r, L = float(prim[1].attrib["radius"]), float(prim[1].attrib["length"])
        half = max(L / 2.0 - r, 0.0)
        axis = Rc @ np.array([0.0, 0.0, 1.0])
    elif prim is not None and prim[0] == "box":
        size = np.asarray(_floats(prim[1].attrib["size"]), dtype=np.float64)
        k = int(np.argmax(size))
        r = float(np.max(np.delete(size, k))) / 2.0
        half = max(size[k] / 2.0 - r, 0.0)
        axis = Rc @ np.eye(3)[k]
    elif prim is not None and prim[0] == "sphere":
        r, half, axis = float(prim[1].attrib["radius"]), 0.0, np.array([0.0, 0.0, 1.0])
    else:
        if cap is not None:   # a capsule fitted to the link's collision mesh (robots/*_link_capsules.json)
            return np.asarray([cap["a"][0], cap["a"][1], cap["a"][2], cap["r"], cap["b"][0], cap["b"][1], cap["b"][2], 0.0],
                              dtype=np.float32)
        b = fallback_b
        return np.asarray([0.0, 0.0, 0.0, default_radius, b[0], b[1], b[2], 0.0], dtype=np.float32)
    a, b = xyz - half * axis, xyz + half * axis
    return np.asarray([a[0], a[1], a[2], r, b[0], b[1], b[2], 0.0], dtype=np.float32)


# ---- self collision: link-vs-link pairs (simulation.py:411-441, helper/pybullet_helper.py:46-68) ----------------------------

def _within_neighborhood(table: KinematicTable, link_a: int, link_b: int, n_neighbors: int) -> bool:
    """check_link_neighborhood: a == b, or one of the two is among the first `n_neighbors` parents of the other (-1 = the base
    link, which has no parent)."""
    if link_a == link_b:
        return True
    for link, other in ((link_a, link_b), (link_b, link_a)):
        elem = link
        for _ in range(n_neighbors):
            if elem == -1:
                break
            parent = int(table.parent[elem])
            if parent == other:
                return True
            elem = parent
    return False


def self_collision_pairs(table: KinematicTable, leaf_frames: Sequence[int], n_neighbors: int = 3,
                         base_has_collision: bool = True):
    """The self pairs of a policy set: [(leaf ordinal, frame B or -1)].  `leaf_frames` are the frames of the leaves that take
    per-pair obstacle data (distance and attached-point maps), in leaf order; ordinal i is leaf_frames[i].  Link A = the leaf's
    link, link B = any other link with a collision shape, the fixed base (-1) included; a pair is dropped when either link is
    within `n_neighbors` parent hops of the other (the reference's rule, both directions as its double loop gives them).  B is
    an obstacle for the step: no derivative flows through it.  Grouped by leaf ordinal, B ascending from -1."""
    out = []
    for i, a in enumerate(leaf_frames):
        a = int(a)
        if not table.has_collision[a]:
            continue
        for b in range(-1, table.n_frames):
            has_b = base_has_collision if b < 0 else bool(table.has_collision[b])
            if not has_b or _within_neighborhood(table, a, b, n_neighbors):
                continue
            out.append((i, b))
    return out


def base_link_name(urdf_filepath: str, table: KinematicTable) -> str:
    """Name of the fixed base link: the parent link of the joints attached to the base (parent[f] == -1)."""
    root = ElementTree.parse(urdf_filepath).getroot()
    roots = [table.frame_names[f] for f in range(table.n_frames) if table.parent[f] < 0]
    for j in root.findall("joint"):
        if j.attrib.get("name") in roots:
            return j.find("parent").attrib["link"]
    raise ValueError("no joint attached to the base link")


def self_collision_capsules(urdf_filepath: str, table: KinematicTable, default_radius: float = 0.06, fitted="auto") -> np.ndarray:
    """Capsules [n_frames + 1, 8] = (a, radius, b, 0) for rmp2_set_self_collision: row f is frame f's link in frame coordinates,
    as link_capsules builds it; the last row is the base link in base coordinates.  Frames without a collision shape get a zero
    row (self_collision_pairs never pairs them)."""
    F = table.n_frames
    out = np.zeros((F + 1, 8), dtype=np.float32)
    frames = [table.frame_names[f] for f in range(F) if table.has_collision[f]]
    if frames:
        rows = link_capsules(urdf_filepath, table, frames, default_radius=default_radius, fitted=fitted)
        for fr, row in zip(frames, rows):
            out[table.frame_index(fr)] = row
    root = ElementTree.parse(urdf_filepath).getroot()
    link_by_name = {l.attrib["name"]: l for l in root.findall("link")}
    base = base_link_name(urdf_filepath, table)
    fitted = fitted_link_capsules(urdf_filepath) if fitted == "auto" else (fitted or {})
    out[F] = _link_capsule(link_by_name.get(base), fitted.get(base), np.zeros(3), default_radius)
    return out


def contact_capsules(urdf_filepath: str, table: KinematicTable, default_radius: float = 0.06, fitted="auto") -> np.ndarray:
    """Capsules [n_frames, 8] for Engine.set_contact_capsules (include/rmp2.h rmp2_set_contact_capsules): rows 0 .. F - 1 of
    self_collision_capsules -- the base link is static and takes no part in the plant's contacts."""
    return np.ascontiguousarray(self_collision_capsules(urdf_filepath, table, default_radius=default_radius, fitted=fitted)[:table.n_frames])


def contact_self_pairs(table: KinematicTable, n_neighbors: int = 3) -> np.ndarray:
    """Frame pairs [n, 2] int32 (i < j) for Engine.set_contact_self_pairs (include/rmp2.h rmp2_set_contact_self_pairs): every two
    frames with a collision shape that are not within `n_neighbors` parent hops of each other, in either direction
    (self_collision_pairs' rule), each unordered pair once; pairs that the same dofs move (rigidly connected: nothing can change
    their gap) are left out.  The static base link takes no part."""
    def dofs(f):
        out = set()
        while f >= 0:
            if int(table.joint_type[f]) != JOINT_FIXED and int(table.q_index[f]) >= 0:
                out.add(int(table.q_index[f]))
            f = int(table.parent[f])
        return out

    frames = [f for f in range(table.n_frames) if table.has_collision[f]]
    out = [(a, b) for k, a in enumerate(frames) for b in frames[k + 1:]
           if not _within_neighborhood(table, a, b, n_neighbors) and dofs(a) != dofs(b)]
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


MAX_CONTACT_PLANES = 8   # include/rmp2.h RMP2_MAX_CONTACT_PLANES


def contact_planes(rows) -> np.ndarray:
    """Half-spaces [P, 4] float32 = (unit normal, d) for Engine.dynamics_step(contact_planes=) (include/rmp2.h
    rmp2_dynamics_step_contacts_planes; free space is n . x >= d) from host rows (nx, ny, nz, d) whose normal may have any length:
    normal and offset are divided by |n| in float64, so the half-space stays the one the row states.  Refused: a zero or
    non-finite normal, a non-finite offset, more than MAX_CONTACT_PLANES rows."""
    a = np.asarray(rows, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 4), np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"contact planes must be rows (nx, ny, nz, d), got shape {list(a.shape)}")
    if len(a) > MAX_CONTACT_PLANES:
        raise ValueError(f"{len(a)} contact planes, at most {MAX_CONTACT_PLANES}")
    if not np.isfinite(a).all():
        raise ValueError("contact planes: a value is not finite")
    length = np.linalg.norm(a[:, :3], axis=1)
    if (length == 0).any():
        raise ValueError(f"contact planes: row {int(np.argmax(length == 0))} has a zero normal")
    out = (a / length[:, None]).astype(np.float32)
    if not np.isfinite(out).all() or (np.abs(out[:, :3]).max(1) == 0).any():
        raise ValueError("contact planes: a row does not normalise in float32")
    return np.ascontiguousarray(out)


def floor(z: float = 0.0) -> np.ndarray:
    """The ground plane at height z as contact_planes' [1, 4]: the reference scenes' plane.urdf."""
    return contact_planes([[0.0, 0.0, 1.0, float(z)]])


MAX_OBSTACLE_CAPSULES = 32   # include/rmp2.h RMP2_MAX_OBSTACLE_CAPSULES


def capsule_obstacles(rows) -> np.ndarray:
    """Capsule obstacles [C, 8] float32 = (a.xyz, radius, b.xyz, 0) for Engine.dynamics_step(contact_obstacle_capsules=)
    (include/rmp2.h rmp2_dynamics_step_contacts_capsules) from host rows of 7 or 8 values -- the record of RMP2_PRIM_CAPSULE tables
    and configs.sample_capsules; the unused eighth word is zeroed.  Refused: a non-finite value, a negative radius, more than
    MAX_OBSTACLE_CAPSULES rows."""
    a = np.asarray(rows, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 8), np.float32)
    if a.ndim != 2 or a.shape[1] not in (7, 8):
        raise ValueError(f"capsule obstacles must be rows (ax, ay, az, radius, bx, by, bz[, 0]), got shape {list(a.shape)}")
    if len(a) > MAX_OBSTACLE_CAPSULES:
        raise ValueError(f"{len(a)} capsule obstacles, at most {MAX_OBSTACLE_CAPSULES}")
    if not np.isfinite(a[:, :7]).all():
        raise ValueError("capsule obstacles: a value is not finite")
    if (a[:, 3] < 0).any():
        raise ValueError(f"capsule obstacles: row {int(np.argmax(a[:, 3] < 0))} has a negative radius")
    out = np.zeros((len(a), 8), np.float32)
    out[:, :7] = a[:, :7]
    if not np.isfinite(out).all():
        raise ValueError("capsule obstacles: a value is not finite in float32")
    return out


def cylinders_as_capsules(cylinders, mode: str = "covering") -> np.ndarray:
    """configs.cylinder_record rows [C, 8] = (centre c, radius r, unit axis u, half-height h) -- the reference's flat-capped
    cylinders -- as capsule_obstacles records, for the plant's contacts (which know capsules only):
      "covering":  end points c -+ h u, radius r.  Contains the cylinder; overshoots each cap by at most r (on the axis).
      "inscribed": end points c -+ max(h - r, 0) u, radius r.  Lies inside the cylinder whenever h >= r; misses the rim by at most
                   (sqrt 2 - 1) r.
    The end points are formed in float64 and rounded once."""
    if mode not in ("covering", "inscribed"):
        raise ValueError(f"mode must be 'covering' or 'inscribed', got {mode!r}")
    a = np.asarray(cylinders, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 8), np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"cylinders must be rows (cx, cy, cz, radius, ux, uy, uz, half_height), got shape {list(a.shape)}")
    if not np.isfinite(a).all():
        raise ValueError("cylinders: a value is not finite")
    c, r, u, h = a[:, 0:3], a[:, 3], a[:, 4:7], a[:, 7]
    if (r < 0).any() or (h < 0).any():
        raise ValueError("cylinders: a negative radius or half-height")
    length = np.linalg.norm(u, axis=1)
    if (length == 0).any():
        raise ValueError(f"cylinders: row {int(np.argmax(length == 0))} has a zero axis")
    u = u / length[:, None]
    reach = h if mode == "covering" else np.maximum(h - r, 0.0)
    return capsule_obstacles(np.concatenate([c - reach[:, None] * u, r[:, None], c + reach[:, None] * u], axis=1))


MAX_OBSTACLE_CYLINDERS = 32   # include/rmp2.h RMP2_MAX_OBSTACLE_CYLINDERS


def cylinder_obstacles(rows) -> np.ndarray:
    """Flat-capped cylinder obstacles [Y, 8] float32 = (centre xyz, radius, unit axis xyz, half height) for
    Engine.dynamics_step(contact_cylinders=) (include/rmp2.h rmp2_dynamics_step_contacts_cylinders) from host rows of 8 values --
    configs.cylinder_record rows, the record of RMP2_PRIM_CYLINDER tables: the table that engine.obstacles(..., primitive="cylinder")
    steers around is the one the plant simulates.  The axis is normalised in float64 (the device uses it as given) and the record
    rounded once.  Refused: a wrong shape, a non-finite value, a zero axis, radius <= 0, half height < 0, more than
    MAX_OBSTACLE_CYLINDERS rows."""
    a = np.asarray(rows, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 8), np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"cylinder obstacles must be rows (cx, cy, cz, radius, ux, uy, uz, half_height), got shape {list(a.shape)}")
    if len(a) > MAX_OBSTACLE_CYLINDERS:
        raise ValueError(f"{len(a)} cylinder obstacles, at most {MAX_OBSTACLE_CYLINDERS}")
    if not np.isfinite(a).all():
        raise ValueError("cylinder obstacles: a value is not finite")
    if (a[:, 3] <= 0).any():
        raise ValueError(f"cylinder obstacles: row {int(np.argmax(a[:, 3] <= 0))} has a radius <= 0")
    if (a[:, 7] < 0).any():
        raise ValueError(f"cylinder obstacles: row {int(np.argmax(a[:, 7] < 0))} has a negative half height")
    length = np.linalg.norm(a[:, 4:7], axis=1)
    if (length == 0).any():
        raise ValueError(f"cylinder obstacles: row {int(np.argmax(length == 0))} has a zero axis")
    out = a.copy()
    out[:, 4:7] /= length[:, None]
    out = out.astype(np.float32)
    if not np.isfinite(out).all():
        raise ValueError("cylinder obstacles: a value is not finite in float32")
    return out


def cylinder_scenes(scenes):
    """Per-robot cylinder scenes as ONE pool and ONE CSR pair: scenes is a sequence of R row arrays [n_r, 8] (cylinder_obstacles'
    rows; configs.cylinder_record / configs.sample_cylinders rows qualify; n_r = 0 allowed) -> (pool [Y, 8] float32, csr_offset
    int32 [R + 1], csr_index int32 [Y]), the scenes' records one after the other and every robot listing its own, ascending.  The
    three arrays feed both Engine.obstacles(spheres=pool, csr_offset=, csr_index=, primitive="cylinder") and
    Engine.dynamics_step(contact_cylinders=pool, contact_cylinder_lists=(csr_offset, csr_index)) (include/rmp2.h
    rmp2_dynamics_step_contacts_cylinder_lists).  Axes are normalised and rows refused as cylinder_obstacles does it -- a robot with
    more than MAX_OBSTACLE_CYLINDERS rows, non-finite values --, a pool beyond 1 << 22 records (RMP2_MAX_CYLINDER_POOL) as well."""
    pools, offset = [], [0]
    for r, rows in enumerate(scenes):
        try:
            pools.append(cylinder_obstacles(rows))
        except ValueError as e:
            raise ValueError(f"cylinder scene of robot {r}: {e}") from None
        offset.append(offset[-1] + len(pools[-1]))
    if offset[-1] > (1 << 22):
        raise ValueError(f"{offset[-1]} cylinders in the pool, at most {1 << 22}")
    pool = np.concatenate(pools).astype(np.float32) if pools else np.zeros((0, 8), np.float32)
    return np.ascontiguousarray(pool.reshape(-1, 8)), np.asarray(offset, np.int32), np.arange(offset[-1], dtype=np.int32)


# ---- convex-hull link geometry (simulation.py:462-484: PyBullet loads each .obj collision mesh as its convex hull) ------------

MAX_HULL_VERTICES = 512   # include/rmp2.h RMP2_MAX_HULL_VERTICES
MAX_HULL_FACES = 1024     # include/rmp2.h RMP2_MAX_HULL_FACES


def read_obj_vertices(path: str) -> np.ndarray:
    """The `v ` lines of a Wavefront .obj as [n, 3] float64."""
    with open(path) as f:
        v = [list(map(float, line.split()[1:4])) for line in f if line.startswith("v ")]
    return np.asarray(v, dtype=np.float64).reshape(-1, 3)


def collision_meshes(urdf_filepath: str) -> dict:
    """{link name: (vertices [n, 3] float64, xyz [3], rpy [3])} for every link whose <collision> geometry is a <mesh>: the
    mesh's vertex set as written in its .obj (`package://` resolved against the URDF's directory) and the collision origin that
    places it on the link.  The package's kinematics-only URDFs have no meshes (an empty dict)."""
    root = ElementTree.parse(urdf_filepath).getroot()
    here = os.path.dirname(os.path.abspath(urdf_filepath))
    out = {}
    for link in root.findall("link"):
        col = link.find("collision")
        geom = col.find("geometry") if col is not None else None
        mesh = geom.find("mesh") if geom is not None else None
        if mesh is None:
            continue
        origin = col.find("origin")
        path = os.path.join(here, mesh.attrib["filename"].replace("package://", ""))
        out[link.attrib["name"]] = (read_obj_vertices(path),
                                    np.asarray(_floats(origin.attrib.get("xyz") if origin is not None else None), dtype=np.float64),
                                    np.asarray(_floats(origin.attrib.get("rpy") if origin is not None else None), dtype=np.float64))
    return out


@dataclass
class LinkHulls:
    """Convex hulls of the pair leaves' links, packed for rmp2_set_link_hulls: hull i (the i-th distance / attached-point leaf
    in leaf order) has vertices verts[vert_offset[i]:vert_offset[i + 1]] and face planes planes[face_offset[i]:face_offset[i + 1]]
    = (n, d) with unit outward n and n . x <= d inside, all in the leaf's FRAME coordinates."""
    vert_offset: np.ndarray   # [L + 1] int32
    verts: np.ndarray         # [V, 3] float32
    face_offset: np.ndarray   # [L + 1] int32
    planes: np.ndarray        # [F, 4] float32

    def __len__(self) -> int:
        return len(self.vert_offset) - 1

    def hull(self, i: int):
        """(vertices [n, 3], planes [m, 4]) of hull i."""
        return (self.verts[self.vert_offset[i]:self.vert_offset[i + 1]], self.planes[self.face_offset[i]:self.face_offset[i + 1]])

    def subset(self, entries: Sequence[int]) -> "LinkHulls":
        """The hulls `entries` (in that order) packed on their own: self_collision_hulls(...).subset(leaf frames) are the
        pair leaves' hulls, bit for bit those link_hulls builds."""
        V = [self.hull(int(e))[0] for e in entries]
        P = [self.hull(int(e))[1] for e in entries]
        vo = np.concatenate([[0], np.cumsum([len(v) for v in V])]).astype(np.int32)
        fo = np.concatenate([[0], np.cumsum([len(p) for p in P])]).astype(np.int32)
        return LinkHulls(vo, np.ascontiguousarray(np.concatenate(V) if V else np.zeros((0, 3)), dtype=np.float32).reshape(-1, 3),
                         fo, np.ascontiguousarray(np.concatenate(P) if P else np.zeros((0, 4)), dtype=np.float32).reshape(-1, 4))


def convex_hull(points: np.ndarray):
    """(vertices [n, 3] float64, planes [m, 4] float64) of the convex hull of `points` [k, 3]: the hull's vertices (a subset of
    the points) and one outward unit plane (n, d), n . x <= d inside, per facet direction (coplanar triangles merged)."""
    from scipy.spatial import ConvexHull   # (setup time only)
    h = ConvexHull(np.asarray(points, dtype=np.float64))
    verts = h.points[h.vertices]
    eq = h.equations            # (n, offset) with n . x + offset <= 0 inside, n unit
    planes = np.concatenate([eq[:, :3], -eq[:, 3:4]], axis=1)
    keep = []
    for p in planes:            # merge the triangles of one facet (same plane to 1e-9)
        if not any(np.abs(p - q).max() <= 1e-9 for q in keep):
            keep.append(p)
    return verts, np.asarray(keep, dtype=np.float64)


def _link_hull(link: str, meshes: dict, what: str):
    """(vertices, planes) float64 of `link`'s convex hull in the coordinates its entry of `meshes` is placed in (link_hulls)."""
    if link not in meshes:
        raise ValueError(f"{what}: no collision mesh for link {link!r}: pass its vertex set in `meshes`")
    m = meshes[link]
    if isinstance(m, (tuple, list)):
        verts, xyz, rpy = m
        Rc = rotation_from_rpy_reference_order(rpy).astype(np.float64)
        pts = np.asarray(verts, dtype=np.float64) @ Rc.T + np.asarray(xyz, dtype=np.float64)
    else:
        pts = np.asarray(m, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or len(pts) < 4:
        raise ValueError(f"{what}: link {link!r} needs at least 4 vertices [n, 3]")
    hv, hp = convex_hull(pts)
    if len(hv) > MAX_HULL_VERTICES or len(hp) > MAX_HULL_FACES:
        raise ValueError(f"{what}: the hull of {link!r} has {len(hv)} vertices / {len(hp)} faces (at most "
                         f"{MAX_HULL_VERTICES} / {MAX_HULL_FACES})")
    return hv, hp


def self_collision_hulls(urdf_filepath: str, table: KinematicTable, meshes: dict) -> LinkHulls:
    """Hulls [n_frames + 1] for rmp2_set_self_collision_hulls, laid out as self_collision_capsules: entry f is frame f's link in
    FRAME coordinates, built exactly as link_hulls builds it (so the pair leaves' entries are bit for bit link_hulls(table,
    leaf frames, meshes)); the last entry is the base link (base_link_name) in base coordinates.  Frames without a collision
    shape get an empty entry (self_collision_pairs never pairs them); a collision frame whose link has no mesh is an error."""
    F = table.n_frames
    links = [table.link_names[f] if table.has_collision[f] else None for f in range(F)] + [base_link_name(urdf_filepath, table)]
    vo, fo, V, P = [0], [0], [], []
    for link in links:
        hv, hp = (np.zeros((0, 3)), np.zeros((0, 4))) if link is None else _link_hull(link, meshes, "self_collision_hulls")
        V.append(hv)
        P.append(hp)
        vo.append(vo[-1] + len(hv))
        fo.append(fo[-1] + len(hp))
    return LinkHulls(np.asarray(vo, np.int32), np.ascontiguousarray(np.concatenate(V), dtype=np.float32).reshape(-1, 3),
                     np.asarray(fo, np.int32), np.ascontiguousarray(np.concatenate(P), dtype=np.float32).reshape(-1, 4))


def link_hulls(table: KinematicTable, frames: Sequence[str], meshes: dict) -> LinkHulls:
    """One convex hull per pair leaf (`frames` in leaf order, as link_capsules takes them), in that leaf's FRAME coordinates:
    the mesh vertices of the frame's link placed by its collision origin (rotation_from_rpy_reference_order, as the fitted
    capsules are), then their convex hull.  `meshes` maps link names to (vertices, xyz, rpy) -- collision_meshes(urdf) -- or to
    a bare [n, 3] vertex set already in link coordinates.  A frame whose link has no entry is an error; so is a hull beyond
    MAX_HULL_VERTICES / MAX_HULL_FACES."""
    vo, fo, V, P = [0], [0], [], []
    for fr in frames:
        link = table.link_names[table.frame_index(fr)]
        if link not in meshes:
            raise ValueError(f"link_hulls: no collision mesh for link {link!r} (frame {fr!r}): pass its vertex set in `meshes`")
        hv, hp = _link_hull(link, meshes, "link_hulls")
        V.append(hv)
        P.append(hp)
        vo.append(vo[-1] + len(hv))
        fo.append(fo[-1] + len(hp))
    return LinkHulls(np.asarray(vo, np.int32), np.ascontiguousarray(np.concatenate(V), dtype=np.float32).reshape(-1, 3),
                     np.asarray(fo, np.int32), np.ascontiguousarray(np.concatenate(P), dtype=np.float32).reshape(-1, 4))


# ---- inertial data (rmp2_set_inertials: the rigid-body model of the inverse dynamics, simulation.py:369-386) -----------------

INERTIAL_FLOATS = 10   # (m, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Ixz, Iyz): include/rmp2.h rmp2_set_inertials


def read_inertials(urdf_filepath: str) -> dict:
    """{link name: (mass, xyz [3], rpy [3], inertia6 [6])} of every link with an <inertial> element: the mass, the inertial origin
    (the centre of mass and the axes the tensor is written in, in link coordinates; 0 where absent) and the tensor as written,
    inertia6 = (ixx, iyy, izz, ixy, ixz, iyz).  A link without <inertial> is massless (the URDF default) and has no entry.  The
    package's kinematics-only URDFs carry no inertials (an empty dict)."""
    root = ElementTree.parse(urdf_filepath).getroot()
    out = {}
    for link in root.findall("link"):
        inr = link.find("inertial")
        if inr is None:
            continue
        origin = inr.find("origin")
        mass = inr.find("mass")
        ten = inr.find("inertia")
        i6 = [float(ten.attrib.get(k, "0")) if ten is not None else 0.0 for k in ("ixx", "iyy", "izz", "ixy", "ixz", "iyz")]
        out[link.attrib["name"]] = (float(mass.attrib["value"]) if mass is not None else 0.0,
                                    np.asarray(_floats(origin.attrib.get("xyz") if origin is not None else None), dtype=np.float64),
                                    np.asarray(_floats(origin.attrib.get("rpy") if origin is not None else None), dtype=np.float64),
                                    np.asarray(i6, dtype=np.float64))
    return out


def read_effort_limits(urdf_filepath: str, order: Sequence[str]) -> np.ndarray:
    """float32 [n]: the <limit effort=> of the joints in `order` (N m, or N for a prismatic joint), inf where the joint has no
    <limit> or the attribute is absent: the tau_limit of Engine.dynamics_step."""
    root = ElementTree.parse(urdf_filepath).getroot()
    joints = {j.attrib["name"]: j for j in root.findall("joint")}
    out = np.full(len(order), np.inf, dtype=np.float32)
    for i, name in enumerate(order):
        if name not in joints:
            raise ValueError(f"{urdf_filepath}: no joint named {name!r}")
        lim = joints[name].find("limit")
        if lim is not None and "effort" in lim.attrib:
            out[i] = float(lim.attrib["effort"])
    return out


def read_joint_limits(urdf_filepath: str, order: Sequence[str]):
    """(lower, upper), float32 [n] each: the <limit lower= upper=> of the joints in `order` (rad, or m for a prismatic joint);
    -inf / +inf for a continuous joint, a joint without <limit> or an absent attribute: the q_limits of Engine.dynamics_step."""
    root = ElementTree.parse(urdf_filepath).getroot()
    joints = {j.attrib["name"]: j for j in root.findall("joint")}
    lower = np.full(len(order), -np.inf, dtype=np.float32)
    upper = np.full(len(order), np.inf, dtype=np.float32)
    for i, name in enumerate(order):
        if name not in joints:
            raise ValueError(f"{urdf_filepath}: no joint named {name!r}")
        lim = joints[name].find("limit")
        if lim is None or joints[name].attrib.get("type") == "continuous":
            continue
        if "lower" in lim.attrib:
            lower[i] = float(lim.attrib["lower"])
        if "upper" in lim.attrib:
            upper[i] = float(lim.attrib["upper"])
    return lower, upper


def inertial_table(table: KinematicTable, inertials: dict) -> np.ndarray:
    """float32 [n_frames, 10] for rmp2_set_inertials: frame f's record describes its child link (table.link_names[f]) in FRAME
    coordinates, (m, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Ixz, Iyz) -- c the centre of mass, the tensor about c in frame axes.
    `inertials` is read_inertials(urdf) (or a dict of the same shape): the tensor is rotated from the inertial origin's axes into
    the frame's, I = R I_origin R^T with R = rotation_from_rpy_reference_order(rpy) -- the convention of the collision origins in
    link_hulls.  The reference's URDFs all have zero inertial rpy, so nothing the reference runs tells that order from the URDF
    standard's apart.  A frame whose link has no entry is massless; the fixed base link's entry plays no part."""
    out = np.zeros((table.n_frames, INERTIAL_FLOATS), dtype=np.float32)
    for f, link in enumerate(table.link_names):
        if link not in inertials:
            continue
        m, xyz, rpy, i6 = inertials[link]
        ixx, iyy, izz, ixy, ixz, iyz = (float(v) for v in i6)
        I = np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]], dtype=np.float64)
        Rm = rotation_from_rpy_reference_order(rpy).astype(np.float64)
        I = Rm @ I @ Rm.T
        c = np.asarray(xyz, dtype=np.float64)
        out[f] = [float(m), c[0], c[1], c[2], I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]
    return out


def panda_table() -> KinematicTable:
    return compile_urdf(PANDA_URDF, PANDA_ORDER)


def two_joint_table() -> KinematicTable:
    return compile_urdf(TWO_JOINT_URDF, TWO_JOINT_ORDER)

"""Time the plant's step with capsule obstacles beside the spheres and the half-spaces (include/rmp2.h
rmp2_dynamics_step_contacts_capsules) against the planes call, on the workload and by the method of
tools/contact_timing_common.py (the fleet, the timing loop, one process per measurement).  Prints ONE JSON line
(profiles/contact_capsules_timing.json).  Per fleet size:
  (a) `planes_us`: the existing rmp2_dynamics_step_contacts_planes on the 32-sphere table with one floor 50 m below.  With
      --parent-lib this leg alternates between the parent's library and this build (`planes_us_parent`, `planes_us_this`,
      `planes_us_ok`: this build's median is not above the parent's largest round plus the parent's own relative spread): the
      kernel is meant to be the parent's.
  (b) `capsules_far_us`: the capsule call on the same scene with seven capsules 50 m away: the capsule trips run, no capsule row
      ever qualifies.  This build only (the parent has no such call).
  (c) `capsules_touch_us`: the capsule call with seven covering capsules (urdf.cylinders_as_capsules) of experiment 06's cylinder
      distribution (configs.sample_cylinders: radius 0.05 .. 0.1, height 0.5, its orientations), each moved beside a link of a
      start state that no earlier capsule is near -- d_act / 2 from the link's middle, across both axes --, so that most robots
      have a capsule candidate at the start (`capsule_fraction`, from the fp64 poses of the start states).
`b_over_a`, `c_over_b`: the ratios of the medians.  `far_same_results`: the final state and status of (b) had the bits of (a)'s.
usage: python tools/contact_capsules_timing.py [--parent-lib PATH] [--rounds N] [steps] [reps]"""
import json

import contact_timing_common as T

FAR_FLOOR = [[0.0, 0.0, 1.0, -50.0]]
N_CAPSULES = 7


def touching_capsules(c):
    """(capsules [7, 8] float32, the fraction of start states with a capsule pair within d_act): see the head."""
    import numpy as np
    import contact_capsules_reference as QR
    import contacts_reference as CR
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    cyl = Cf.sample_cylinders(np.random.default_rng(606), N_CAPSULES).astype(np.float64)
    q0 = np.asarray(c.q0, np.float64)
    Rw, pw, _ = CR.poses(c.table, q0)
    frames = [f for f in CR.capsule_frames(c.caps) if (c.caps[f, 0:3] != c.caps[f, 4:7]).any()]
    covered = np.zeros(len(q0), bool)
    for j in range(N_CAPSULES):
        i = int(np.argmin(covered))          # (the first start state that no capsule is near yet)
        f = frames[(len(frames) // 2 + j) % len(frames)]
        a, b = c.caps[f, 0:3].astype(np.float64), c.caps[f, 4:7].astype(np.float64)
        X0, D = Rw[f][i] @ (0.5 * (a + b)) + pw[f][i], Rw[f][i] @ (b - a)
        m = np.cross(D, cyl[j, 4:7])
        m = m / np.linalg.norm(m) if np.linalg.norm(m) > 1e-6 else np.array([0.0, 0.0, 1.0])
        cyl[j, 0:3] = X0 + m * (c.caps[f, 3] + cyl[j, 3] + 0.5 * T.D_ACT)
        one = U.cylinders_as_capsules(cyl[j:j + 1])
        covered |= QR.capsule_rows(c.table, c.caps, one, 0, 0, q0)["gap"].min(1) <= T.D_ACT
    capsules = U.cylinders_as_capsules(cyl)
    near = QR.capsule_rows(c.table, c.caps, capsules, 0, 0, q0)["gap"].min(1) <= T.D_ACT
    return capsules, round(float(near.mean()), 4)


def call(c, planes, capsules=None):
    c.eng.dynamics_step(c.qs, c.qds, c.u, T.DT, stop_out=c.stop, status_out=c.status, contacts=c.spheres, d_act=T.D_ACT,
                        contact_planes=planes, **({} if capsules is None else {"contact_obstacle_capsules": capsules}), **c.step)


def planes(c):
    import torch
    floor = torch.tensor(FAR_FLOOR, device=c.dev)
    c.time("planes_us", lambda: call(c, floor))
    c.final("planes_bits", lambda: call(c, floor))
    c.row["contact_fraction"] = round(float((c.status.cpu().numpy() & 4 != 0).mean()), 4)


def capsules(c, touching):
    import numpy as np
    import torch
    floor = torch.tensor(FAR_FLOOR, device=c.dev)
    key = "capsules_touch" if touching else "capsules_far"
    if touching:
        table, fraction = touching_capsules(c)
    else:
        table = np.array([[50.0 + j, 3.0, 1.0, 0.05 + 0.01 * j, 50.0 + j, 3.0, 1.5, 0.0] for j in range(N_CAPSULES)], np.float32)
    oc = torch.from_numpy(table).to(c.dev)
    c.time(key + "_us", lambda: call(c, floor, oc))
    c.final(key + "_bits", lambda: call(c, floor, oc))
    if touching:
        st = c.status.cpu().numpy()
        c.row["capsule_fraction"] = fraction
        c.row["contact_fraction_touch"] = round(float((st & 4 != 0).mean()), 4)
        c.row["overflow_fraction_touch"] = round(float((st & 8 != 0).mean()), 4)
        c.row["finite_touch"] = bool(torch.isfinite(c.qs).all())


LEGS = {"planes": planes, "capsules_far": lambda c: capsules(c, False), "capsules_touch": lambda c: capsules(c, True)}
parent_lib, rounds, child, steps, reps = T.parse(__doc__)
if child is not None:
    T.main(__file__, "contact_capsules_timing", LEGS, __doc__)          # (measures the leg, prints its rows and exits)
result = T.main(__file__, "contact_capsules_timing", {"planes": planes}, __doc__)          # (a): alternating with the parent's library
for name in ("capsules_far", "capsules_touch"):          # (b), (c): this build only
    for row, got in zip(result["sizes"], T.run_child(__file__, name, steps, reps)):
        row.update({k: v for k, v in got.items() if k != "robots"})
for row in result["sizes"]:
    row["far_same_results"] = row["planes_bits"] == row["capsules_far_bits"]
    row["b_over_a"] = round(row["capsules_far_us"] / row["planes_us"], 3)
    row["c_over_b"] = round(row["capsules_touch_us"] / row["capsules_far_us"], 3)
print(json.dumps(result))

"""Time the plant's step with half-space obstacles beside the spheres (include/rmp2.h rmp2_dynamics_step_contacts_planes) against
the shared-table sphere call, on the workload and by the method of tools/contact_timing_common.py (the fleet, the timing loop,
--parent-lib and what it adds to every leg).  Prints ONE JSON line (profiles/contact_planes_timing.json).  Per fleet size:
  (a) `shared_us`: rmp2_dynamics_step_contacts on the 32-sphere table.
  (b) `planes_far_us`: the planes call on the same table with one floor 50 m below the lowest link: the plane trip runs, no
      plane row ever qualifies.
  (c) `planes_touch_us`: the planes call with the floor at the fleet's own lower-quartile height of the lowest capsule end of the
      links that two or more joints move (fp64 poses of the start states) minus d_act / 2: the low links of about a quarter of the
      robots are within d_act of it or below it at the start (`floor_fraction`), and their plane rows enter the solver.
`b_over_a`, `c_over_b`: the ratios of the medians.  `far_same_results`: the final state and status of (b) had the bits of (a)'s.
usage: python tools/contact_planes_timing.py [--parent-lib PATH] [--rounds N] [steps] [reps]"""
import json

import contact_timing_common as T


def _anc_mask(table, f):
    """Bit j: dof j's joint is frame f's or an ancestor's."""
    m = 0
    while f >= 0:
        if table.joint_type[f] != 0 and table.q_index[f] >= 0:
            m |= 1 << int(table.q_index[f])
        f = int(table.parent[f])
    return m


def floors(c):
    """(far, touch, the fraction of start states within d_act of `touch` or below it): the floors' heights, from the lowest
    capsule end (surface) of every start state among the links that two or more joints move (the first link only turns about the
    vertical: its height never changes), fp64."""
    import numpy as np
    import contacts_reference as CR
    Rw, pw, _ = CR.poses(c.table, c.q0)
    low = np.full(len(c.q0), np.inf)
    for f in CR.capsule_frames(c.caps):
        if bin(_anc_mask(c.table, f)).count("1") < 2:
            continue
        for end in (c.caps[f, 0:3], c.caps[f, 4:7]):
            low = np.minimum(low, (Rw[f] @ end.astype(np.float64) + pw[f])[:, 2] - c.caps[f, 3])
    touch = float(np.percentile(low, 25) - T.D_ACT / 2)
    return float(low.min() - 50.0), touch, round(float((low - touch <= T.D_ACT).mean()), 4)


def call(c, planes=None):
    c.eng.dynamics_step(c.qs, c.qds, c.u, T.DT, stop_out=c.stop, status_out=c.status, contacts=c.spheres, d_act=T.D_ACT,
                        **({} if planes is None else {"contact_planes": planes}), **c.step)


def shared(c):
    c.time("shared_us", lambda: call(c))
    c.final("shared_bits", lambda: call(c))
    c.row["contact_fraction"] = round(float((c.status.cpu().numpy() & 4 != 0).mean()), 4)


def planes(c, touching):
    import torch
    far, touch, fraction = floors(c)
    key = "planes_touch" if touching else "planes_far"
    floor = torch.tensor([[0.0, 0.0, 1.0, touch if touching else far]], device=c.dev)
    c.time(key + "_us", lambda: call(c, floor))
    c.final(key + "_bits", lambda: call(c, floor))
    c.row["floor_" + key[7:] + "_z"] = round(touch if touching else far, 4)
    if touching:
        st = c.status.cpu().numpy()
        c.row["floor_fraction"] = fraction
        c.row["contact_fraction_touch"] = round(float((st & 4 != 0).mean()), 4)
        c.row["overflow_fraction_touch"] = round(float((st & 8 != 0).mean()), 4)
        c.row["finite_touch"] = bool(torch.isfinite(c.qs).all())


result = T.main(__file__, "contact_planes_timing",
                {"shared": shared, "planes_far": lambda c: planes(c, False), "planes_touch": lambda c: planes(c, True)}, __doc__)
for row in result["sizes"]:
    row["far_same_results"] = row["shared_bits"] == row["planes_far_bits"]
    row["b_over_a"] = round(row["planes_far_us"] / row["shared_us"], 3)
    row["c_over_b"] = round(row["planes_touch_us"] / row["planes_far_us"], 3)
print(json.dumps(result))

"""Time the plant's step with obstacle contacts (include/rmp2.h rmp2_dynamics_step_contacts) on the workload and by the method of
tools/contact_timing_common.py (the fleet, the timing loop, --parent-lib and what it adds to every leg).  Prints ONE JSON line
(profiles/contacts_timing.json).  Per fleet size:
  (a) `stops_us`: rmp2_dynamics_step_stops, an entry point beside the contacts.
  (b) `contacts_far_us`: the contact call with the 32 spheres moved 50 m away: the candidate search, no candidate.
  (c) `contacts_mix_us`: the contact call on the table itself, and beside it `contact_fraction` / `stop_fraction` (robots with a
      contact / a stop active in some substep), `overflow`, `capped` and `iteration_histogram` (robots by the largest iteration
      count of a substep).
usage: python tools/contacts_timing.py [--parent-lib PATH] [--rounds N] [steps] [reps]"""
import json

import contact_timing_common as T


def stops(c):
    c.time("stops_us", lambda: c.eng.dynamics_step(c.qs, c.qds, c.u, T.DT, stop_out=c.stop, status_out=c.status, **c.step))


def call(c, tab):
    c.eng.dynamics_step(c.qs, c.qds, c.u, T.DT, stop_out=c.stop, status_out=c.status, contacts=tab, d_act=T.D_ACT, **c.step)


def far(c):
    tab = c.spheres.clone()
    tab[:, 0] += 50.0
    c.time("contacts_far_us", lambda: call(c, tab))
    c.final("contacts_far_bits", lambda: call(c, tab))
    assert int((c.status & 12).max()) == 0


def mix(c):
    import numpy as np
    c.time("contacts_mix_us", lambda: call(c, c.spheres))
    c.final("contacts_mix_bits", lambda: call(c, c.spheres))
    st = c.status.cpu().numpy()
    c.row["contact_fraction"] = round(float((st & 4 != 0).mean()), 4)
    c.row["stop_fraction"] = round(float((st & 1 != 0).mean()), 4)
    c.row["overflow"] = int((st & 8 != 0).sum())
    c.row["capped"] = int((st & 2 != 0).sum())
    c.row["iteration_histogram"] = np.bincount(st >> 8).tolist()


print(json.dumps(T.main(__file__, "contacts_timing", {"stops": stops, "far": far, "mix": mix}, __doc__)))

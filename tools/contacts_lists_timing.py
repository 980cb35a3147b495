"""Time the plant's step with per-robot obstacle lists (include/rmp2.h rmp2_dynamics_step_contacts_lists) against the shared-table
call on the same spheres, on the workload and by the method of tools/contact_timing_common.py (the fleet, the timing loop,
--parent-lib and what it adds to every leg).  Prints ONE JSON line (profiles/contacts_lists_timing.json).  Per fleet size:
  (a) `shared_us`: rmp2_dynamics_step_contacts on the 32-sphere table.
  (b) `lists_same_us`: the list call, every robot's list = 0 .. 31 over that same table: every lane gathers the same addresses.
  (c) `lists_own_us`: the list call, robot r's list = 32 r .. 32 r + 31 over a pool of R x 32 records (the same 32 spheres
      replicated): every lane gathers its own 512 bytes.
`b_over_a`, `c_over_b`: the ratios of the medians.  The three legs compute the same numbers: `same_results` says that the final
state and status of (b) and (c) had the bits of (a)'s.
usage: python tools/contacts_lists_timing.py [--parent-lib PATH] [--rounds N] [steps] [reps]"""
import json

import contact_timing_common as T


def call(c, tab, lists=None):
    c.eng.dynamics_step(c.qs, c.qds, c.u, T.DT, stop_out=c.stop, status_out=c.status, contacts=tab, d_act=T.D_ACT,
                        **({} if lists is None else {"contact_lists": lists}), **c.step)


def shared(c):
    c.time("shared_us", lambda: call(c, c.spheres))
    c.final("shared_bits", lambda: call(c, c.spheres))
    c.row["contact_fraction"] = round(float((c.status.cpu().numpy() & 4 != 0).mean()), 4)


def lists(c, own):
    import torch
    off = torch.arange(c.R + 1, dtype=torch.int32, device=c.dev) * T.SPHERES
    if own:
        idx, pool = torch.arange(c.R * T.SPHERES, dtype=torch.int32, device=c.dev), c.spheres.repeat(c.R, 1).contiguous()
        c.row["pool_bytes_own"] = int(pool.numel() * 4)
    else:
        idx, pool = torch.arange(T.SPHERES, dtype=torch.int32, device=c.dev).repeat(c.R), c.spheres
    key = "lists_own" if own else "lists_same"
    c.time(key + "_us", lambda: call(c, pool, (off, idx)))
    c.final(key + "_bits", lambda: call(c, pool, (off, idx)))
    c.row[key + "_invalid"] = int((c.status.cpu().numpy() & 16 != 0).sum())


result = T.main(__file__, "contacts_lists_timing",
                {"shared": shared, "lists_same": lambda c: lists(c, False), "lists_own": lambda c: lists(c, True)}, __doc__)
for row in result["sizes"]:
    row["same_results"] = row["shared_bits"] == row["lists_same_bits"] == row["lists_own_bits"]
    row["b_over_a"] = round(row["lists_same_us"] / row["shared_us"], 3)
    row["c_over_b"] = round(row["lists_own_us"] / row["lists_same_us"], 3)
print(json.dumps(result))

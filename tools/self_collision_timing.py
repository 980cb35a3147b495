"""Time the self-collision route (include/rmp2.h rmp2_set_self_collision): config 3 at 65 536 robots, solve = pinv, the 44 self
pairs of the reference's rule, without and with the 32-sphere table plus link capsules.  Prints ONE JSON line.

Per case: `step_us` = rmp2_step with self collision on (the stage + the explicit-pair step: two launches); `explicit_step_us` = the
explicit-pair step alone on the same pair arrays (a handle without self collision); `stage_us` = their difference; `self_pairs_us`
= rmp2_self_pairs on its own (no table).  Medians over `reps` timed repeats of `steps` back-to-back launches after a warm-up;
HIP events around each repeat.  Bytes: the stage writes p_link + p_obs (24 B per pair) and the explicit-pair step reads them
back; the fraction is of 8 TB/s for that traffic over stage_us + explicit_step_us.
usage: python tools/self_collision_timing.py [R] [steps] [reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U  # noqa: E402
from riemannian_motion_policies_amd.engine import Engine  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 15
dev = torch.device("cuda", 0)
table, desc = Cf.config3("pinv")
leaf_frames = [desc.leaves[i].frame for i in D.distance_leaf_indices(desc)]
pairs = U.self_collision_pairs(table, leaf_frames)
caps = U.self_collision_capsules(U.PANDA_URDF, table)
eng, plain = Engine(desc, 0), Engine(desc, 0)
eng.set_self_collision(pairs, caps)
counts = eng.self_counts
s = Cf.sample_panda_states(np.random.default_rng(1), R)
q, qd, goal = (torch.from_numpy(s[k]).to(dev) for k in ("q", "qd", "goal"))
lc = torch.from_numpy(U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)).to(dev)
sp = torch.from_numpy(Cf.sample_spheres(np.random.default_rng(7), Cf.N_SPHERES)).to(dev)


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / steps * 1e3)
    return float(np.median(per)), float(np.min(per)), float(np.max(per))


result = {"tool": "self_collision_timing", "config": "config3", "solve": "pinv", "robots": R, "self_pairs": len(pairs),
          "steps_per_repeat": steps, "repeats": reps, "cases": []}
self_us = timed(lambda: eng.self_pairs(q))
result["self_pairs_us"] = round(self_us[0], 2)
for name, obst, K in (("self only", None, 0), ("self + 32 spheres + link capsules", eng.obstacles(spheres=sp, link_capsules=lc), 32)):
    out = torch.empty_like(q)
    step_us = timed(lambda: eng.step(q, qd, goal, obstacles=obst, out=out))
    # the same pair arrays for a handle without self collision
    spl, spo, _ = eng.self_pairs(q)
    if K:
        opl, opo = eng.closest_points(q, eng.obstacles(spheres=sp), link_capsules=lc)
        pl = torch.cat([t for i, c in enumerate(counts) for t in (opl[:, i * K:(i + 1) * K], spl[:, sum(counts[:i]):sum(counts[:i + 1])])], 1)
        po = torch.cat([t for i, c in enumerate(counts) for t in (opo[:, i * K:(i + 1) * K], spo[:, sum(counts[:i]):sum(counts[:i + 1])])], 1)
    else:
        pl, po = spl, spo
    pl, po = pl.contiguous(), po.contiguous()
    ob_plain = plain.obstacles(p_link=pl, p_obs=po, pair_counts=[K + c for c in counts])
    explicit_us = timed(lambda: plain.step(q, qd, goal, obstacles=ob_plain, out=out))
    P = pl.shape[1]
    pair_bytes = R * P * 24
    stage_us = step_us[0] - explicit_us[0]
    result["cases"].append({
        "case": name, "pairs_per_robot": int(P), "bytes_per_robot": int(P * 24),
        "step_us": round(step_us[0], 2), "step_us_min_max": [round(step_us[1], 2), round(step_us[2], 2)],
        "explicit_step_us": round(explicit_us[0], 2), "stage_us": round(stage_us, 2),
        "pair_bytes_written_and_read": 2 * pair_bytes,
        "stage_write_TBps": round(pair_bytes / stage_us / 1e6, 3) if stage_us > 0 else None,
        "fraction_of_8TBps": round(2 * pair_bytes / step_us[0] / 1e6 / 8.0, 3),
        "kernel": eng.last_kernel()})
print(json.dumps(result))

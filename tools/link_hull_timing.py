"""Time the convex-hull link geometry (include/rmp2.h rmp2_set_link_hulls): config 3 at 65 536 robots, solve = pinv, a table of
32 spheres, the Panda's collision-mesh hulls (tests/golden/panda_collision_meshes.npz through urdf.link_hulls).  Prints ONE JSON
line and writes it to profiles/link_hull_timing.json.

`hull_stage_us` = rmp2_closest_points_hulls alone; `hull_step_us` = rmp2_step on the handle with hulls (the stage + the
explicit-pair step: two launches); `capsule_step_us` = the same step with link_capsules instead (the fused capsule form, a handle
without hulls); `capsule_stage_us` = rmp2_closest_points_links with the capsules.  Medians over `reps` timed repeats of `steps`
back-to-back launches after a warm-up; HIP events around each repeat.
usage: python tools/link_hull_timing.py [R] [steps] [reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from riemannian_motion_policies_amd import configs as Cf, urdf as U  # noqa: E402
from riemannian_motion_policies_amd.engine import Engine  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
dev = torch.device("cuda", 0)
table, desc = Cf.config3("pinv")
z = np.load(os.path.join(ROOT, "tests", "golden", "panda_collision_meshes.npz"))
meshes = {str(n): (z[f"{n}.vertices"], z[f"{n}.xyz"], z[f"{n}.rpy"]) for n in z["links"]}
hulls = U.link_hulls(table, Cf.CONTROL_POINT_FRAMES, meshes)
eng, plain = Engine(desc, 0), Engine(desc, 0)
eng.set_link_hulls(hulls)
s = Cf.sample_panda_states(np.random.default_rng(1), R)
q, qd, goal = (torch.from_numpy(s[k]).to(dev) for k in ("q", "qd", "goal"))
lc = torch.from_numpy(U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)).to(dev)
sp = torch.from_numpy(Cf.sample_spheres(np.random.default_rng(7), Cf.N_SPHERES)).to(dev)


def timed(fn):
    for _ in range(3):
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
    return round(float(np.median(per)), 2), [round(float(np.min(per)), 2), round(float(np.max(per)), 2)]


tab = eng.obstacles(spheres=sp)
out = torch.empty_like(q)
pl = torch.empty((R, 8 * Cf.N_SPHERES, 3), device=dev)
res = {"tool": "link_hull_timing", "config": "config3", "solve": "pinv", "robots": R, "spheres": Cf.N_SPHERES,
       "hull_vertices": [int(x) for x in np.diff(hulls.vert_offset)], "hull_faces": [int(x) for x in np.diff(hulls.face_offset)],
       "steps_per_repeat": steps, "repeats": reps}
res["hull_stage_us"], res["hull_stage_us_min_max"] = timed(lambda: eng.closest_points_hulls(q, tab))
res["hull_step_us"], res["hull_step_us_min_max"] = timed(lambda: eng.step(q, qd, goal, obstacles=tab, out=out))
res["hull_step_kernel"] = eng.last_kernel()
ob_caps = plain.obstacles(spheres=sp, link_capsules=lc)
res["capsule_step_us"], res["capsule_step_us_min_max"] = timed(lambda: plain.step(q, qd, goal, obstacles=ob_caps, out=out))
res["capsule_step_kernel"] = plain.last_kernel()
res["capsule_stage_us"], _ = timed(lambda: plain.closest_points(q, plain.obstacles(spheres=sp), link_capsules=lc))
line = json.dumps(res)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "link_hull_timing.json"), "w") as f:
    f.write(line + "\n")

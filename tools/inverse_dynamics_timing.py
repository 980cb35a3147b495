"""Time the inverse dynamics (include/rmp2.h rmp2_inverse_dynamics) on the config-3 Panda with the reference's inertials
(tests/golden/robot_inertials.npz) at 4 096 and 65 536 robots.  Prints ONE JSON line (profiles/inverse_dynamics_timing.json).

Per fleet size: `inverse_dynamics_us` = rmp2_inverse_dynamics alone; `forward_kinematics_us` = rmp2_forward_kinematics at the same
size (the walk it is compared with); `step_us` = rmp2_step (config 3: 32 shared spheres, solve = pinv as bench.py runs it);
`step_then_inverse_dynamics_us` = rmp2_step followed by rmp2_inverse_dynamics on its qdd, on one stream.  Medians over `reps`
timed repeats of `steps` back-to-back launches after a warm-up; HIP events around each repeat.
usage: python tools/inverse_dynamics_timing.py [steps] [reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from riemannian_motion_policies_amd import configs as Cf, urdf as U  # noqa: E402
from riemannian_motion_policies_amd.engine import Engine  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda", 0)
table, desc = Cf.config3("pinv")
z = np.load(os.path.join(ROOT, "tests", "golden", "robot_inertials.npz"))
inertials = {str(n): (float(z["panda.mass"][i]), z["panda.xyz"][i], z["panda.rpy"][i], z["panda.inertia6"][i])
             for i, n in enumerate(z["panda.links"])}
eng = Engine(desc, 0)
eng.set_inertials(U.inertial_table(table, inertials))


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


result = {"tool": "inverse_dynamics_timing", "config": "config3", "solve": "pinv", "steps_per_repeat": steps, "repeats": reps,
          "bytes_per_robot": 4 * 4 * desc.robot.n_dof, "sizes": []}
for R in (4096, 65536):
    s = Cf.sample_panda_states(np.random.default_rng(1), R)
    q, qd, goal = (torch.from_numpy(s[k]).to(dev) for k in ("q", "qd", "goal"))
    obs = eng.obstacles(spheres=torch.from_numpy(Cf.sample_spheres(np.random.default_rng(7), Cf.N_SPHERES)))
    qdd = torch.empty_like(q)
    tau = torch.empty_like(q)
    eng.step(q, qd, goal, obstacles=obs, out=qdd)
    row = {"robots": R}
    row["inverse_dynamics_us"], row["inverse_dynamics_us_min_max"] = timed(lambda: eng.inverse_dynamics(q, qd, qdd, out=tau))
    row["forward_kinematics_us"], _ = timed(lambda: eng.forward_kinematics(q))
    row["step_us"], _ = timed(lambda: eng.step(q, qd, goal, obstacles=obs, out=qdd))
    row["step_then_inverse_dynamics_us"], row["step_then_inverse_dynamics_us_min_max"] = timed(
        lambda: (eng.step(q, qd, goal, obstacles=obs, out=qdd), eng.inverse_dynamics(q, qd, qdd, out=tau)))
    row["kernel"] = eng.last_kernel()
    row["inverse_dynamics_GBps"] = round(result["bytes_per_robot"] * R / row["inverse_dynamics_us"] / 1e3, 1)
    result["sizes"].append(row)
print(json.dumps(result))

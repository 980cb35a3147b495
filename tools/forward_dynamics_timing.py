"""Time the plant (include/rmp2.h rmp2_mass_matrix / rmp2_forward_dynamics / rmp2_dynamics_step) on the config-3 Panda with the
reference's inertials (tests/golden/robot_inertials.npz) at 4 096 and 65 536 robots.  Prints ONE JSON line
(profiles/forward_dynamics_timing.json).

Per fleet size: `mass_matrix_us`, `forward_dynamics_us` (torques = the inverse dynamics of the step's qdd), `dynamics_step_us`
for 10 substeps in the acceleration drive without limits (nothing saturates: ten walks, no solve), with the Panda URDF's effort
limits (`dynamics_step_limited_us`, with the fraction of robots that saturate at the first substep) and in the torque drive (ten
walks, ten solves); for scale `inverse_dynamics_us` and `step_us` = rmp2_step (config 3: 32 shared spheres, solve = pinv as
bench.py runs it) in the same call.  Medians over `reps` timed repeats of `steps` back-to-back launches after a warm-up; HIP events
around each repeat.  The stepped state is reset before every repeat (a copy outside the timed span).
usage: python tools/forward_dynamics_timing.py [steps] [reps]"""
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
SUBSTEPS, DT = 10, 0.001
dev = torch.device("cuda", 0)
table, desc = Cf.config3("pinv")
z = np.load(os.path.join(ROOT, "tests", "golden", "robot_inertials.npz"))
inertials = {str(n): (float(z["panda.mass"][i]), z["panda.xyz"][i], z["panda.rpy"][i], z["panda.inertia6"][i])
             for i, n in enumerate(z["panda.links"])}
eng = Engine(desc, 0)
eng.set_inertials(U.inertial_table(table, inertials))
limits = torch.from_numpy(U.read_effort_limits(U.PANDA_URDF, U.PANDA_ORDER)).to(dev)


def timed(fn, reset=None):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(reps):
        if reset is not None:
            reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / steps * 1e3)
    return round(float(np.median(per)), 2), [round(float(np.min(per)), 2), round(float(np.max(per)), 2)]


result = {"tool": "forward_dynamics_timing", "config": "config3", "solve": "pinv", "steps_per_repeat": steps, "repeats": reps,
          "substeps": SUBSTEPS, "dt": DT, "sizes": []}
for R in (4096, 65536):
    s = Cf.sample_panda_states(np.random.default_rng(1), R)
    q, qd, goal = (torch.from_numpy(s[k]).to(dev) for k in ("q", "qd", "goal"))
    obs = eng.obstacles(spheres=torch.from_numpy(Cf.sample_spheres(np.random.default_rng(7), Cf.N_SPHERES)))
    qdd = torch.empty_like(q)
    tau = torch.empty_like(q)
    out = torch.empty_like(q)
    M = torch.empty((R, desc.robot.n_dof, desc.robot.n_dof), device=dev)
    qs, qds = q.clone(), qd.clone()
    eng.step(q, qd, goal, obstacles=obs, out=qdd)
    eng.inverse_dynamics(q, qd, qdd, out=tau)

    def reset():
        qs.copy_(q)
        qds.copy_(qd)

    row = {"robots": R}
    row["mass_matrix_us"], row["mass_matrix_us_min_max"] = timed(lambda: eng.mass_matrix(q, out=M))
    row["forward_dynamics_us"], row["forward_dynamics_us_min_max"] = timed(lambda: eng.forward_dynamics(q, qd, tau, out=out))
    row["dynamics_step_us"], row["dynamics_step_us_min_max"] = timed(
        lambda: eng.dynamics_step(qs, qds, qdd, DT, substeps=SUBSTEPS), reset)
    row["dynamics_step_limited_us"], row["dynamics_step_limited_us_min_max"] = timed(
        lambda: eng.dynamics_step(qs, qds, qdd, DT, substeps=SUBSTEPS, tau_limit=limits), reset)
    row["saturated_fraction"] = round(float(((tau.abs() > limits).any(1)).float().mean()), 4)
    row["dynamics_step_torque_us"], row["dynamics_step_torque_us_min_max"] = timed(
        lambda: eng.dynamics_step(qs, qds, tau, DT, substeps=SUBSTEPS, drive="torque"), reset)
    row["inverse_dynamics_us"], _ = timed(lambda: eng.inverse_dynamics(q, qd, qdd, out=tau))
    row["step_us"], _ = timed(lambda: eng.step(q, qd, goal, obstacles=obs, out=qdd))
    row["kernel"] = eng.last_kernel()
    result["sizes"].append(row)
print(json.dumps(result))

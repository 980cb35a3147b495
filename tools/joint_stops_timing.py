"""Time the plant's step with joint-limit stops (include/rmp2.h rmp2_dynamics_step_stops) on the Panda with the reference's
inertials at 4 096 and 65 536 robots, by the method of tools/forward_dynamics_timing.py: medians over `reps` timed repeats of
`steps` launches of 10 substeps after a warm-up.  Unlike there, the stepped state is reset before EVERY launch, outside the
launch's own pair of HIP events (a repeat's figure is the mean over its launches): stepped on, a fleet leans on its stops, and
the timed mix would not be the one the histogram describes.  Prints ONE JSON line (profiles/joint_stops_timing.json).

The fleet is the tests' (tests/test_joint_stops_host.py stop_fleet: of every four robots one clear of its limits, one with a
single joint about to meet a stop, two with a third of their joints about to; 4 096 states, tiled to the fleet size), in the
acceleration drive against the URDF's effort limits, dt = 0.01.  Per fleet size:
  (a) `dynamics_step_us`: rmp2_dynamics_step, the unchanged entry point.  With --parent-lib (a library built from the parent
      commit) the measurement alternates between that library and this build, `rounds` times each, every measurement in a
      process of its own (RMP2_LIB picks the library); `parent_us` / `this_us` list them in order.
  (b) `stops_far_us`: the stops call with limits nobody comes near (+-1e3): the fast path on every robot.
  (c) `stops_mix_us`: the stops call with the Panda's limits, and beside it `active_fraction` (robots with some stop active in
      some substep), `capped` and `iteration_histogram` (robots by the largest iteration count of a substep).
usage: python tools/joint_stops_timing.py [--parent-lib PATH] [--rounds N] [steps] [reps]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

args = sys.argv[1:]
parent_lib, rounds, child = None, 3, None
while args and args[0].startswith("--"):
    flag = args.pop(0)
    if flag == "--parent-lib":
        parent_lib = os.path.abspath(args.pop(0))
    elif flag == "--rounds":
        rounds = int(args.pop(0))
    elif flag == "--child":
        child = args.pop(0)
    else:
        sys.exit(__doc__)
steps = int(args[0]) if len(args) > 0 else 20
reps = int(args[1]) if len(args) > 1 else 7
SUBSTEPS, DT, SIZES, STATES = 10, 0.01, (4096, 65536), 4096


def run_child(what, lib=None):
    env = dict(os.environ)
    if lib is not None:
        env["RMP2_LIB"] = lib
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(steps), str(reps)], env=env,
                          capture_output=True, text=True, timeout=900)
    if done.returncode != 0:
        sys.exit(f"measurement {what!r} (library: {lib or 'this build'}) failed with {done.returncode}:\n{done.stderr[-2000:]}")
    return json.loads(done.stdout.strip().splitlines()[-1])


def measure(what):
    import numpy as np
    import torch
    import test_joint_stops_host as S
    import joint_stops_reference as JR
    from test_inverse_dynamics_host import fixture_inertials
    from riemannian_motion_policies_amd import descriptor as D, urdf as U
    from riemannian_motion_policies_amd.engine import Engine

    dev = torch.device("cuda", 0)
    table = U.panda_table()
    inert = U.inertial_table(table, fixture_inertials(os.path.join(ROOT, "tests", "golden"), "panda"))
    eng = Engine(D.build_desc(table, []), 0)
    eng.set_inertials(inert)
    effort = torch.from_numpy(U.read_effort_limits(U.PANDA_URDF, U.PANDA_ORDER)).to(dev)
    lo, hi = (torch.from_numpy(x).to(dev) for x in JR.table_limits(table))
    far_lo, far_hi = torch.full_like(lo, -1e3), torch.full_like(hi, 1e3)
    q0, qd0, u0 = S.stop_fleet(np.random.default_rng(400), table, inert, (0.0, 0.0, -9.81), STATES, DT)

    def timed(fn, reset):
        """Every launch starts from the reset state (the copy is outside its pair of events), so that all `steps` launches of a
        repeat run the same mix; a repeat's figure is the mean over its launches."""
        for _ in range(3):
            reset()
            fn()
        torch.cuda.synchronize()
        per = []
        for _ in range(reps):
            events = []
            for _ in range(steps):
                reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                events.append((e0, e1))
            torch.cuda.synchronize()
            per.append(sum(a.elapsed_time(b) for a, b in events) / steps * 1e3)
        return round(float(np.median(per)), 2), [round(float(np.min(per)), 2), round(float(np.max(per)), 2)]

    rows = []
    for R in SIZES:
        q, qd, u = (torch.from_numpy(np.tile(x, (R // STATES, 1))).to(dev) for x in (q0, qd0, u0))
        qs, qds = q.clone(), qd.clone()

        def reset():
            qs.copy_(q)
            qds.copy_(qd)

        row = {"robots": R}
        if what == "plain":
            row["dynamics_step_us"], row["dynamics_step_us_min_max"] = timed(
                lambda: eng.dynamics_step(qs, qds, u, DT, substeps=SUBSTEPS, tau_limit=effort), reset)
        else:
            status = torch.zeros(R, dtype=torch.int32, device=dev)
            stop = torch.empty_like(q)
            row["stops_far_us"], row["stops_far_us_min_max"] = timed(
                lambda: eng.dynamics_step(qs, qds, u, DT, substeps=SUBSTEPS, tau_limit=effort, q_limits=(far_lo, far_hi),
                                          stop_out=stop, status_out=status), reset)
            torch.cuda.synchronize()
            assert int(status.max()) == 0
            row["stops_mix_us"], row["stops_mix_us_min_max"] = timed(
                lambda: eng.dynamics_step(qs, qds, u, DT, substeps=SUBSTEPS, tau_limit=effort, q_limits=(lo, hi), stop_out=stop,
                                          status_out=status), reset)
            reset()
            eng.dynamics_step(qs, qds, u, DT, substeps=SUBSTEPS, tau_limit=effort, q_limits=(lo, hi), stop_out=stop, status_out=status)
            torch.cuda.synchronize()
            st = status.cpu().numpy()
            row["active_fraction"] = round(float((st & 1 != 0).mean()), 4)
            row["capped"] = int((st & 2 != 0).sum())
            row["iteration_histogram"] = np.bincount(st >> 8).tolist()
        rows.append(row)
    return rows


if child is not None:
    print(json.dumps(measure(child)))
    sys.exit(0)

result = {"tool": "joint_stops_timing", "robot": "panda", "drive": "accel", "tau_limit": "urdf effort", "steps_per_repeat": steps,
          "repeats": reps, "substeps": SUBSTEPS, "dt": DT, "parent_lib": bool(parent_lib), "sizes": [{"robots": R} for R in SIZES]}
runs = {"parent": [], "this": []}
for _ in range(rounds if parent_lib else 1):
    if parent_lib:
        runs["parent"].append(run_child("plain", parent_lib))
    runs["this"].append(run_child("plain"))
stops = run_child("stops")
for i, row in enumerate(result["sizes"]):
    for who in ("parent", "this"):
        if runs[who]:
            row[f"{who}_us"] = [r[i]["dynamics_step_us"] for r in runs[who]]
            row[f"{who}_us_min_max"] = [min(r[i]["dynamics_step_us_min_max"][0] for r in runs[who]),
                                        max(r[i]["dynamics_step_us_min_max"][1] for r in runs[who])]
    row["dynamics_step_us"] = sorted(row["this_us"])[len(row["this_us"]) // 2]
    row.update({k: v for k, v in stops[i].items() if k != "robots"})
print(json.dumps(result))

"""Time the plant's step with obstacle contacts (include/rmp2.h rmp2_dynamics_step_contacts) on the Panda with the reference's
inertials at 4 096 and 65 536 robots, by the method of tools/joint_stops_timing.py: medians over `reps` timed repeats of `steps`
launches of 10 substeps after a warm-up, the stepped state reset before EVERY launch, outside the launch's own pair of HIP
events.  Prints ONE JSON line (profiles/contacts_timing.json).

The fleet is the tests' (tests/test_contacts_host.py contact_fleet: of every four robots three near a base state that touches two
or three spheres of the shared table, one clear of it; 4 096 states, tiled to the fleet size) on a table of 32 spheres, in the
acceleration drive against the URDF's effort limits, with the Panda's joint limits, dt = 0.01, d_act = 0.03.  Per fleet size:
  (a) `stops_us`: rmp2_dynamics_step_stops, the unchanged entry point.  With --parent-lib (a library built from the parent
      commit) the measurement alternates between that library and this build, `rounds` times each, every measurement in a
      process of its own (RMP2_LIB picks the library); `parent_us` / `this_us` list them in order.
  (b) `contacts_far_us`: the contact call with the same 32 spheres moved 50 m away: the candidate search, no candidate.
  (c) `contacts_mix_us`: the contact call on the table itself, and beside it `contact_fraction` / `stop_fraction` (robots with a
      contact / a stop active in some substep), `overflow`, `capped` and `iteration_histogram` (robots by the largest iteration
      count of a substep).
usage: python tools/contacts_timing.py [--parent-lib PATH] [--rounds N] [steps] [reps]"""
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
SUBSTEPS, DT, SIZES, STATES, SPHERES, D_ACT = 10, 0.01, (4096, 65536), 4096, 32, 0.03


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
    import test_contacts_host as S
    caps = S.robot_capsules("panda")
    q0, qd0, u0, spheres = S.contact_fleet(np.random.default_rng(600), table, inert, (0.0, 0.0, -9.81), caps, STATES, SPHERES)

    def timed(fn, reset):
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
        status = torch.zeros(R, dtype=torch.int32, device=dev)
        stop = torch.empty_like(q)
        if what == "stops":
            row["stops_us"], row["stops_us_min_max"] = timed(
                lambda: eng.dynamics_step(qs, qds, u, DT, substeps=SUBSTEPS, tau_limit=effort, q_limits=(lo, hi), stop_out=stop,
                                          status_out=status), reset)
        else:
            eng.set_contact_capsules(caps)
            sph = torch.from_numpy(spheres).to(dev)
            far = sph.clone()
            far[:, 0] += 50.0

            def call(tab):
                eng.dynamics_step(qs, qds, u, DT, substeps=SUBSTEPS, tau_limit=effort, q_limits=(lo, hi), stop_out=stop,
                                  status_out=status, contacts=tab, d_act=D_ACT)

            row["contacts_far_us"], row["contacts_far_us_min_max"] = timed(lambda: call(far), reset)
            torch.cuda.synchronize()
            assert int((status & 12).max()) == 0
            row["contacts_mix_us"], row["contacts_mix_us_min_max"] = timed(lambda: call(sph), reset)
            reset()
            call(sph)
            torch.cuda.synchronize()
            st = status.cpu().numpy()
            row["contact_fraction"] = round(float((st & 4 != 0).mean()), 4)
            row["stop_fraction"] = round(float((st & 1 != 0).mean()), 4)
            row["overflow"] = int((st & 8 != 0).sum())
            row["capped"] = int((st & 2 != 0).sum())
            row["iteration_histogram"] = np.bincount(st >> 8).tolist()
        rows.append(row)
    return rows


if child is not None:
    print(json.dumps(measure(child)))
    sys.exit(0)

result = {"tool": "contacts_timing", "robot": "panda", "drive": "accel", "tau_limit": "urdf effort", "steps_per_repeat": steps,
          "repeats": reps, "substeps": SUBSTEPS, "dt": DT, "spheres": SPHERES, "d_act": D_ACT, "parent_lib": bool(parent_lib),
          "sizes": [{"robots": R} for R in SIZES]}
runs = {"parent": [], "this": []}
for _ in range(rounds if parent_lib else 1):
    if parent_lib:
        runs["parent"].append(run_child("stops", parent_lib))
    runs["this"].append(run_child("stops"))
contacts = run_child("contacts")
for i, row in enumerate(result["sizes"]):
    for who in ("parent", "this"):
        if runs[who]:
            row[f"{who}_us"] = [r[i]["stops_us"] for r in runs[who]]
            row[f"{who}_us_min_max"] = [min(r[i]["stops_us_min_max"][0] for r in runs[who]),
                                        max(r[i]["stops_us_min_max"][1] for r in runs[who])]
    row["stops_us"] = sorted(row["this_us"])[len(row["this_us"]) // 2]
    row.update({k: v for k, v in contacts[i].items() if k != "robots"})
print(json.dumps(result))

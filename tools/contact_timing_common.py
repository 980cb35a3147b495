"""What tools/contacts_timing.py, tools/contacts_lists_timing.py and tools/contact_planes_timing.py share: the command line, the
fleet, the timing loop and the alternation between two libraries.

The workload: the Panda with the reference's inertials at 4 096 and 65 536 robots, acceleration drive against the URDF's effort
limits, the Panda's joint limits, 10 substeps of 0.01, d_act = 0.03; the tests' fleet (tests/test_contacts_host.py contact_fleet:
of every four robots three near a base state that touches two or three spheres of a table of 32, one clear of it; 4 096 states
tiled to the fleet size).  A measurement is the median over `reps` timed repeats of `steps` launches after a warm-up, the stepped
state reset before EVERY launch, outside the launch's own pair of HIP events.

Every leg of a tool is measured in a process of its own (`--child LEG`; RMP2_LIB picks the library).  With --parent-lib (a library
built from the parent commit; it loads under this tree's Python as long as the ABI has not moved) every leg alternates between that
library and this build, `rounds` times each: per leg and timed key the result holds `<key>_parent` and `<key>_this` (the rounds in
order), `<key>` (the median of this build's rounds) and `<key>_ok`: the median does not exceed the parent's largest round by more
than the parent's own relative spread over its rounds, (max - min) / median -- the noise the run itself shows."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SUBSTEPS, DT, SIZES, STATES, SPHERES, D_ACT = 10, 0.01, (4096, 65536), 4096, 32, 0.03


def parse(doc):
    """(parent_lib, rounds, child, steps, reps) of `[--parent-lib PATH] [--rounds N] [steps] [reps]`."""
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
            sys.exit(doc)
    return parent_lib, rounds, child, int(args[0]) if len(args) > 0 else 20, int(args[1]) if len(args) > 1 else 7


def run_child(script, what, steps, reps, lib=None):
    env = dict(os.environ)
    if lib is not None:
        env["RMP2_LIB"] = lib
    done = subprocess.run([sys.executable, os.path.abspath(script), "--child", what, str(steps), str(reps)], env=env,
                          capture_output=True, text=True, timeout=900)
    if done.returncode != 0:
        sys.exit(f"measurement {what!r} (library: {lib or 'this build'}) failed with {done.returncode}:\n{done.stderr[-2000:]}")
    return json.loads(done.stdout.strip().splitlines()[-1])


def fleet():
    """(dev, engine with inertials and capsules, table, caps, (q0, qd0, u0, spheres), the step's shared keywords)."""
    import numpy as np
    import torch
    import joint_stops_reference as JR
    import test_contacts_host as S
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
    caps = S.robot_capsules("panda")
    eng.set_contact_capsules(caps)
    states = S.contact_fleet(np.random.default_rng(600), table, inert, (0.0, 0.0, -9.81), caps, STATES, SPHERES)
    return dev, eng, table, caps, states, dict(substeps=SUBSTEPS, tau_limit=effort, q_limits=(lo, hi))


def timed(fn, reset, steps, reps):
    """(median, [min, max]) in microseconds per launch."""
    import numpy as np
    import torch
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


def measure(leg, steps, reps):
    """The child's rows, one per fleet size: leg(ctx) fills ctx.row; ctx has dev, eng, table, caps, spheres (tensor), R, q / qd / u
    (the start state), qs / qds (the stepped state), reset(), stop / status, step (the shared keywords), time(key, fn),
    final(key, fn), q0."""
    import numpy as np
    import torch
    from types import SimpleNamespace
    dev, eng, table, caps, (q0, qd0, u0, spheres), step = fleet()
    rows = []
    for R in SIZES:
        q, qd, u = (torch.from_numpy(np.tile(x, (R // STATES, 1))).to(dev) for x in (q0, qd0, u0))
        c = SimpleNamespace(dev=dev, eng=eng, table=table, caps=caps, q0=q0, spheres=torch.from_numpy(spheres).to(dev), R=R, q=q, qd=qd,
                            u=u, qs=q.clone(), qds=qd.clone(), stop=torch.empty_like(q), step=step, row={"robots": R},
                            status=torch.zeros(R, dtype=torch.int32, device=dev))

        def reset(c=c):
            c.qs.copy_(c.q)
            c.qds.copy_(c.qd)

        def time(key, fn, c=c):
            c.row[key], c.row[key + "_min_max"] = timed(fn, c.reset, steps, reps)

        def final(key, fn, c=c):
            """row[key]: a digest of the state and status words that one launch of fn leaves."""
            import hashlib
            c.reset()
            fn()
            torch.cuda.synchronize()
            c.row[key] = hashlib.sha256(c.qs.cpu().numpy().tobytes() + c.qds.cpu().numpy().tobytes()
                                        + c.status.cpu().numpy().tobytes()).hexdigest()[:16]

        c.reset, c.time, c.final = reset, time, final
        leg(c)
        rows.append(c.row)
    return rows


def main(script, tool, legs, doc):
    """legs: {name: leg(ctx)}.  Runs the child named on the command line and exits, or every leg (alternating, see the head) and
    returns the tool's result, for the tool to add its ratios and print as ONE JSON line.  A key that ends in `_bits` is a
    digest (ctx.final): `<key>_as_parent` says that every round of both libraries gave the same one."""
    parent_lib, rounds, child, steps, reps = parse(doc)
    if child is not None:
        print(json.dumps(measure(legs[child], steps, reps)))
        sys.exit(0)
    result = {"tool": tool, "robot": "panda", "drive": "accel", "tau_limit": "urdf effort", "steps_per_repeat": steps, "repeats": reps,
              "substeps": SUBSTEPS, "dt": DT, "spheres": SPHERES, "d_act": D_ACT, "parent_lib": bool(parent_lib),
              "sizes": [{"robots": R} for R in SIZES]}
    for name in legs:
        runs = {"parent": [], "this": []}
        for _ in range(rounds if parent_lib else 1):
            if parent_lib:
                runs["parent"].append(run_child(script, name, steps, reps, parent_lib))
            runs["this"].append(run_child(script, name, steps, reps))
        for i, row in enumerate(result["sizes"]):
            last = runs["this"][-1][i]
            row.update({k: v for k, v in last.items() if k != "robots"})
            for key in [k for k in last if k.endswith("_us")]:
                this = [r[i][key] for r in runs["this"]]
                row[key] = sorted(this)[len(this) // 2]
                row[key + "_min_max"] = [min(r[i][key + "_min_max"][0] for r in runs["this"]),
                                         max(r[i][key + "_min_max"][1] for r in runs["this"])]
                if parent_lib:
                    par = [r[i][key] for r in runs["parent"]]
                    row[key + "_parent"], row[key + "_this"] = par, this
                    spread = (max(par) - min(par)) / sorted(par)[len(par) // 2]
                    row[key + "_ok"] = bool(row[key] <= max(par) * (1.0 + spread))
            for key in [k for k in last if k.endswith("_bits")]:
                if parent_lib:
                    row[key + "_as_parent"] = len({r[i][key] for who in runs for r in runs[who]}) == 1
    return result

"""Time the plant's step with half-space obstacles beside the spheres (include/rmp2.h rmp2_dynamics_step_contacts_planes) against
the shared-table sphere call, in the form of tools/contacts_timing.py and tools/contacts_lists_timing.py: the Panda with the
reference's inertials at 4 096 and 65 536 robots, acceleration drive against the URDF's effort limits, the Panda's joint limits,
10 substeps of 0.01, d_act = 0.03; medians over `reps` timed repeats of `steps` launches after a warm-up, the stepped state reset
before EVERY launch, outside the launch's own pair of HIP events.  Prints ONE JSON line (profiles/contact_planes_timing.json).

The fleet is tools/contacts_timing.py's (of every four robots three near a base state that touches two or three spheres of a
table of 32, one clear of it; 4 096 states tiled to the fleet size).  Per fleet size:
  (a) `shared_us`: rmp2_dynamics_step_contacts on the 32-sphere table -- the unchanged entry point.  With --parent-lib (a library
      built from the parent commit) the measurement alternates between that library and this build, `rounds` times each, every
      measurement in a process of its own (RMP2_LIB picks the library); `parent_us` / `this_us` list them in order.
  (b) `planes_far_us`: the planes call on the same table with one floor 50 m below the lowest link: the plane trip runs, no
      plane row ever qualifies.
  (c) `planes_touch_us`: the planes call with the floor at the fleet's own lower-quartile height of the lowest capsule end of the
      links that two or more joints move (fp64 poses of the start states) minus d_act / 2: the low links of about a quarter of the robots are within d_act of it or
      below it at the start (`floor_fraction`), and their plane rows enter the solver.
`b_over_a`, `c_over_b`: the ratios of the medians.  `far_same_results`: the final q and status of (b) had the bits of (a)'s.
usage: python tools/contact_planes_timing.py [--parent-lib PATH] [--rounds N] [steps] [reps]"""
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


def _anc_mask(table, f):
    """Bit j: dof j's joint is frame f's or an ancestor's."""
    m = 0
    while f >= 0:
        if table.joint_type[f] != 0 and table.q_index[f] >= 0:
            m |= 1 << int(table.q_index[f])
        f = int(table.parent[f])
    return m


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
    eng.set_contact_capsules(caps)
    q0, qd0, u0, spheres = S.contact_fleet(np.random.default_rng(600), table, inert, (0.0, 0.0, -9.81), caps, STATES, SPHERES)

    # the lowest capsule end (surface) of every start state among the links that two or more joints move (the first link only
    # turns about the vertical: its height never changes), fp64
    import contacts_reference as CR
    Rw, pw, _ = CR.poses(table, q0)
    low = np.full(len(q0), np.inf)
    for f in CR.capsule_frames(caps):
        if bin(_anc_mask(table, f)).count("1") < 2:
            continue
        for end in (caps[f, 0:3], caps[f, 4:7]):
            low = np.minimum(low, (Rw[f] @ end.astype(np.float64) + pw[f])[:, 2] - caps[f, 3])
    floor_far = float(low.min() - 50.0)
    floor_touch = float(np.percentile(low, 25) - D_ACT / 2)
    floor_fraction = round(float((low - floor_touch <= D_ACT).mean()), 4)

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
        sph = torch.from_numpy(spheres).to(dev)

        def call(tab, planes=None):
            eng.dynamics_step(qs, qds, u, DT, substeps=SUBSTEPS, tau_limit=effort, q_limits=(lo, hi), stop_out=stop,
                              status_out=status, contacts=tab, d_act=D_ACT, **({} if planes is None else {"contact_planes": planes}))

        def final(tab, planes=None):
            reset()
            call(tab, planes)
            torch.cuda.synchronize()
            return qs.clone(), status.clone()

        if what == "shared":
            row["shared_us"], row["shared_us_min_max"] = timed(lambda: call(sph), reset)
        else:
            far, touch = (torch.tensor([[0.0, 0.0, 1.0, z]], device=dev) for z in (floor_far, floor_touch))
            row["planes_far_us"], row["planes_far_us_min_max"] = timed(lambda: call(sph, far), reset)
            row["planes_touch_us"], row["planes_touch_us_min_max"] = timed(lambda: call(sph, touch), reset)
            qa, sa = final(sph)
            qb, sb = final(sph, far)
            qc, sc = final(sph, touch)
            row["far_same_results"] = bool(torch.equal(qa.view(torch.int32), qb.view(torch.int32)) and torch.equal(sa, sb))
            row["contact_fraction"] = round(float((sa.cpu().numpy() & 4 != 0).mean()), 4)
            row["contact_fraction_touch"] = round(float((sc.cpu().numpy() & 4 != 0).mean()), 4)
            row["overflow_fraction_touch"] = round(float((sc.cpu().numpy() & 8 != 0).mean()), 4)
            row["finite_touch"] = bool(torch.isfinite(qc).all())
            row["floor_far_z"], row["floor_touch_z"], row["floor_fraction"] = round(floor_far, 4), round(floor_touch, 4), floor_fraction
        rows.append(row)
    return rows


if child is not None:
    print(json.dumps(measure(child)))
    sys.exit(0)

result = {"tool": "contact_planes_timing", "robot": "panda", "drive": "accel", "tau_limit": "urdf effort", "steps_per_repeat": steps,
          "repeats": reps, "substeps": SUBSTEPS, "dt": DT, "spheres": SPHERES, "d_act": D_ACT, "parent_lib": bool(parent_lib),
          "sizes": [{"robots": R} for R in SIZES]}
runs = {"parent": [], "this": []}
for _ in range(rounds if parent_lib else 1):
    if parent_lib:
        runs["parent"].append(run_child("shared", parent_lib))
    runs["this"].append(run_child("shared"))
planes = run_child("planes")
for i, row in enumerate(result["sizes"]):
    for who in ("parent", "this"):
        if runs[who]:
            row[f"{who}_us"] = [r[i]["shared_us"] for r in runs[who]]
            row[f"{who}_us_min_max"] = [min(r[i]["shared_us_min_max"][0] for r in runs[who]),
                                        max(r[i]["shared_us_min_max"][1] for r in runs[who])]
    row["shared_us"] = sorted(row["this_us"])[len(row["this_us"]) // 2]
    row.update({k: v for k, v in planes[i].items() if k != "robots"})
    row["b_over_a"] = round(row["planes_far_us"] / row["shared_us"], 3)
    row["c_over_b"] = round(row["planes_touch_us"] / row["planes_far_us"], 3)
    if parent_lib:
        row["a_inside_parent_spread"] = bool(row["parent_us_min_max"][0] <= row["shared_us"] <= row["parent_us_min_max"][1])
print(json.dumps(result))

"""Time the hull self-pair route (include/rmp2.h rmp2_set_self_collision_hulls): config 3 at 65 536 robots, solve = pinv, the 44
self pairs of the reference's rule on the Panda's collision hulls, without and with the 32-sphere table (whose obstacle pairs are
then formed on the same leaf hulls).  Prints ONE JSON line.

Per case: `step_us` = rmp2_step with hull self pairs on (the hull obstacle stage when there is a table, the hull self stage, the
explicit-pair step); `explicit_step_us` = the explicit-pair step alone on the same pair arrays (a handle without self collision);
`stage_us` = their difference.  `self_pairs_us` = rmp2_self_pairs on its own, `obstacle_stage_us` = rmp2_closest_points_hulls on
a handle whose link hulls are the leaf hulls.  Medians over `reps` timed repeats of `steps` back-to-back launches after a warm-up;
HIP events around each repeat.
Face rule: how many (robot, pair) entries and how many (wave, pair) entries -- a wave is 64 consecutive robots -- take the face
rule, counted on the first `face_robots` robots with the fp64 restatement (tests/hull_pair_reference.py).  Only pairs whose
capsules overlap are candidates (capsules contain their hulls), so the count is exact for those robots.
usage: python tools/self_hull_timing.py [R] [steps] [reps] [face_robots]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U  # noqa: E402
from riemannian_motion_policies_amd.engine import Engine  # noqa: E402
import hull_pair_reference as HP  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
face_robots = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
WAVE = 64
dev = torch.device("cuda", 0)
table, desc = Cf.config3("pinv")
leaf_frames = [desc.leaves[i].frame for i in D.distance_leaf_indices(desc)]
pairs = U.self_collision_pairs(table, leaf_frames)
z = np.load(os.path.join(ROOT, "tests", "golden", "panda_collision_meshes.npz"))
hulls = U.self_collision_hulls(U.PANDA_URDF, table, {str(n): (z[f"{n}.vertices"], z[f"{n}.xyz"], z[f"{n}.rpy"]) for n in z["links"]})
eng, plain, lh = Engine(desc, 0), Engine(desc, 0), Engine(desc, 0)
eng.set_self_collision_hulls(pairs, hulls)
lh.set_link_hulls(hulls.subset(leaf_frames))
counts = eng.self_counts
s = Cf.sample_panda_states(np.random.default_rng(1), R)
q, qd, goal = (torch.from_numpy(s[k]).to(dev) for k in ("q", "qd", "goal"))
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
    return float(np.median(per)), float(np.min(per)), float(np.max(per))


result = {"tool": "self_hull_timing", "config": "config3", "solve": "pinv", "robots": R, "self_pairs": len(pairs),
          "steps_per_repeat": steps, "repeats": reps, "cases": []}
result["self_pairs_us"] = round(timed(lambda: eng.self_pairs(q))[0], 2)
result["obstacle_stage_us"] = round(timed(lambda: lh.closest_points_hulls(q, lh.obstacles(spheres=sp)))[0], 2)
for name, obst, K in (("self hull pairs only", None, 0), ("self hull pairs + 32 spheres on the same hulls", eng.obstacles(spheres=sp), 32)):
    out = torch.empty_like(q)
    step_us = timed(lambda: eng.step(q, qd, goal, obstacles=obst, out=out))
    spl, spo, _ = eng.self_pairs(q)
    if K:
        opl, opo, _ = lh.closest_points_hulls(q, lh.obstacles(spheres=sp))
        so = [sum(counts[:i]) for i in range(len(counts) + 1)]
        pl = torch.cat([t for i in range(len(counts)) for t in (opl[:, i * K:(i + 1) * K], spl[:, so[i]:so[i + 1]])], 1)
        po = torch.cat([t for i in range(len(counts)) for t in (opo[:, i * K:(i + 1) * K], spo[:, so[i]:so[i + 1]])], 1)
    else:
        pl, po = spl, spo
    pl, po = pl.contiguous(), po.contiguous()
    ob_plain = plain.obstacles(p_link=pl, p_obs=po, pair_counts=[K + c for c in counts])
    explicit_us = timed(lambda: plain.step(q, qd, goal, obstacles=ob_plain, out=out))
    result["cases"].append({
        "case": name, "pairs_per_robot": int(pl.shape[1]),
        "step_us": round(step_us[0], 2), "step_us_min_max": [round(step_us[1], 2), round(step_us[2], 2)],
        "explicit_step_us": round(explicit_us[0], 2), "stage_us": round(step_us[0] - explicit_us[0], 2),
        "kernel": eng.last_kernel()})

# face rule: capsule-overlapping candidates, decided by the restatement
from test_gpu_self_collision import self_pairs_np  # noqa: E402
import oracle as O  # noqa: E402
n = min(face_robots, R) // WAVE * WAVE
qs = s["q"][:n]
caps = U.self_collision_capsules(U.PANDA_URDF, table)
_, _, _, cgap = self_pairs_np(desc, pairs, caps, qs)
order = [pairs[k] for k in sorted(range(len(pairs)), key=lambda k: pairs[k][0])]
T = O.forward_kinematics(desc, qs, "f64")
F = desc.robot.n_frames
face = np.zeros((n, len(order)), bool)
cache = {}
for r, j in zip(*np.nonzero(cgap < 1e-7)):
    o, b = order[j]
    fa, eb = leaf_frames[o], (F if b < 0 else b)
    for e in (fa, eb):
        if e not in cache:
            cache[e] = HP.Hull(*hulls.hull(e))
    TA, TB = T[r, fa], (np.eye(4) if b < 0 else T[r, b])
    Rm, t = TA[:3, :3].T @ TB[:3, :3], TA[:3, :3].T @ (TB[:3, 3] - TA[:3, 3])
    face[r, j] = HP.pair_closest(cache[fa], cache[eb], Rm, t)[4]
waves = face.reshape(n // WAVE, WAVE, len(order)).any(1)
result["face_rule"] = {
    "robots_checked": int(n), "capsule_overlaps": int((cgap < 1e-7).sum()),
    "pair_share": round(float(face.mean()), 6), "wave_pair_share": round(float(waves.mean()), 6),
    "per_pair": {f"{o},{b}": {"pair_share": round(float(face[:, j].mean()), 5), "wave_share": round(float(waves[:, j].mean()), 5)}
                 for j, (o, b) in enumerate(order) if face[:, j].any()}}
print(json.dumps(result))

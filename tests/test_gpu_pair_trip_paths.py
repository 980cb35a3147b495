"""The trip loops of the culled pair phase (csrc/rmp2_quad.h pair_loop_culled): pass 1 marks the primitives of a 32-record chunk
that are in range of a control point, pass 2 deals the marked pairs to the lanes of the robot, one pair per lane and trip.  The
loop is tested at the bottom, with the first pair taken in front of it, so the cases here are the ways into and out of it: a
chunk without any trip, a chunk in which every lane works on every trip, tables with a second chunk (partial and full), ragged
lists as a membership mask and as a list walk, a capsule table (records fetched a trip ahead) and the 16-lane mapping.

Every case runs the Panda config-3 set through Engine at a fleet size with a partial last wave (300 = 18 waves of 16 robots and
one of 12), in the four-wave build the default benchmark runs and in the build the dispatch picks for the size, and every robot
has to pass oracle.accuracy_gate (no robot exempted, rejected == 0).  The pair counts of the constructed tables are pinned by a
test that needs no GPU (oracle forward kinematics in fp64): the tables exercise the paths named above only while those hold."""
import os

import numpy as np
import pytest

R = 300           # 18 full waves and one of 12 robots
C0 = 0.5          # ObstacleAvoidance: margin + metric_modulation_radius (configs.OBSTACLE_AVOIDANCE_PARAMS[0] + [7])
HAND = 5          # index of panda_hand_joint in configs.CONTROL_POINT_FRAMES


def _states():
    from riemannian_motion_policies_amd import configs as Cf
    return Cf.sample_panda_states(np.random.default_rng(4242), R)


def _origins(desc, q):
    """Control-point positions [R, 8, 3] of the config-3 set (oracle FK, fp64)."""
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd.urdf import panda_table
    t = panda_table()
    frames = [t.frame_index(fr) for fr in Cf.CONTROL_POINT_FRAMES]
    return O.forward_kinematics(desc, q, precision="f64")[:, frames][:, :, :3, 3]


def _in_range(org, table, scale=1.0):
    """[R, 8, K] bool: is primitive k in range of control point (r, f)?  Spheres: |p - c| <= radius + C0; capsules: the
    bounding sphere the kernel tests (centre = midpoint of the axis, radius = half length + capsule radius)."""
    table = np.asarray(table, np.float64)
    if table.shape[1] == 8:
        ctr = 0.5 * (table[:, 0:3] + table[:, 4:7])
        rad = 0.5 * np.linalg.norm(table[:, 4:7] - table[:, 0:3], axis=1) + table[:, 3]
    else:
        ctr, rad = table[:, 0:3], table[:, 3]
    dist = np.linalg.norm(org[:, :, None, :] - ctr[None, None, :, :], axis=-1)
    return dist <= scale * (rad + C0)[None, None, :]


def _far_table():
    """32 spheres five metres above the robots: no control point in range of any."""
    sph = np.zeros((32, 4), np.float32)
    sph[:, 0] = np.linspace(-0.8, 0.8, 32)
    sph[:, 2] = 5.0
    sph[:, 3] = 0.08
    return sph


def _hand_table(org):
    """32 small spheres on a shell of 0.36 .. 0.48 m around robot 0's hand frame, on the side away from the robot's base: all 32
    in range of that control point (eight trips of its quad, every lane with a pair on every trip)."""
    rng = np.random.default_rng(77)
    p = org[0, HAND]
    d = rng.normal(size=(32, 3))
    d[:, 0] = np.abs(d[:, 0])                    # away from the base (the hand is in front of it)
    d[:, 2] = np.abs(d[:, 2])                    # and upward
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sph = np.empty((32, 4), np.float32)
    sph[:, :3] = p[None, :] + d * rng.uniform(0.36, 0.48, (32, 1))
    sph[:, 3] = 0.02
    return sph


def _sphere_table(K):
    from riemannian_motion_policies_amd import configs as Cf
    return Cf.sample_spheres(np.random.default_rng(503 + K), K)


def _capsule_table():
    from riemannian_motion_policies_amd import configs as Cf
    return Cf.sample_capsules(np.random.default_rng(600), 32)


def _ragged(repeat):
    """Per-robot lists over the 32-sphere table: without a repeated index every wave turns its lists into membership masks;
    with the first entry of every non-empty list repeated at its end no list is a mask and every wave walks its lists."""
    from riemannian_motion_policies_amd import configs as Cf
    off, idx = Cf.sample_ragged(np.random.default_rng(700), R, 32)
    if not repeat:
        return off, idx
    lists = [list(idx[off[r]:off[r + 1]]) for r in range(R)]
    lists = [l + l[:1] for l in lists]
    off2 = np.zeros(R + 1, np.int32)
    off2[1:] = np.cumsum([len(l) for l in lists])
    return off2, np.asarray([i for l in lists for i in l], np.int32)


def _listed_pairs(inr, off, idx):
    """In-range pairs of the robots' lists (a repeated index counts twice, as it does in the step)."""
    return int(sum(inr[r][:, idx[off[r]:off[r + 1]]].sum() for r in range(R)))


def _trips(inr):
    """Trips of the quad mapping over one chunk: the most pairs a (robot, frame) of a wave has, in fours, summed over waves and
    frames."""
    per = inr.sum(axis=2)                                                  # [R, 8]
    waves = [per[w:w + 16] for w in range(0, R, 16)]
    return int(sum(((wv.max(axis=0) + 3) // 4).sum() for wv in waves))


def test_pair_counts_of_the_constructed_tables():
    """No GPU: the tables do what the cases are named for.  Counts of |p - c| <= radius + C0 from oracle FK in fp64 (the kernel's
    own test carries 1e-4 of slack and evaluates the pairs inside the slack to an exact zero, so its counts are a few higher)."""
    from riemannian_motion_policies_amd import configs as Cf
    _, desc = Cf.config3()
    s = _states()
    org = _origins(desc, s["q"])
    assert R % 16 == 12

    def counts(table, sl=slice(None)):
        return int(_in_range(org, table)[:, :, sl].sum())

    assert counts(_far_table()) == 0
    assert int(_in_range(org, _far_table(), 2.0).sum()) == 0               # (not even at twice the range)
    hand = _hand_table(org)
    inr = _in_range(org, hand)
    assert inr[0, HAND].all() and _in_range(org, hand, 0.95)[0, HAND].all()  # all 32 in range of robot 0's hand frame
    assert (np.linalg.norm(hand[:, :3] - org[0, HAND], axis=1) - hand[:, 3]).min() > 0.33
    assert counts(hand) == PINNED["hand"]
    for K in (33, 40, 64):
        tab = _sphere_table(K)
        first, second = counts(tab, slice(0, 32)), counts(tab, slice(32, K))
        assert (first, second) == PINNED[K], (K, first, second)
        assert _trips(_in_range(org, tab)[:, :, 32:K]) == PINNED_TRIPS_SECOND_CHUNK[K]
    tab = _sphere_table(32)
    inr = _in_range(org, tab)
    assert counts(tab) == PINNED[32] and _trips(inr) == PINNED_TRIPS[32]
    off, idx = _ragged(False)
    assert all(len(set(idx[off[r]:off[r + 1]])) == off[r + 1] - off[r] for r in range(R))     # masks
    assert (off[1:] == off[:-1]).sum() == PINNED["empty lists"]
    assert _listed_pairs(inr, off, idx) == PINNED["mask"]
    off2, idx2 = _ragged(True)
    assert all(any(len(set(idx2[off2[r]:off2[r + 1]])) < off2[r + 1] - off2[r] for r in range(w, min(w + 16, R)))
               for w in range(0, R, 16))                                                      # every wave walks its lists
    assert int((off2[1:] - off2[:-1]).max()) == 33                                            # a list beyond one chunk
    assert _listed_pairs(inr, off2, idx2) == PINNED["list"]
    assert counts(_capsule_table()) == PINNED["capsules"]


# in-range (control point, primitive) pairs of the tables above over the 300 robots x 8 frames (first chunk, second chunk)
PINNED = {"hand": 41344, 33: (18500, 1471), 40: (14379, 5122), 64: (14471, 12550), 32: 18965, "empty lists": 10, "mask": 9007,
          "list": 9566, "capsules": 40918}
# trips of the quad mapping those pairs make (the most pairs of a (robot, frame) of a wave, in fours)
PINNED_TRIPS = {32: 452}
PINNED_TRIPS_SECOND_CHUNK = {33: 133, 40: 214, 64: 344}


def _engine(desc, kernel, minw):
    """Engine under RMP2_KERNEL / RMP2_QUAD_MINW (both read when the handle is created)."""
    from riemannian_motion_policies_amd.engine import Engine
    want = {"RMP2_KERNEL": kernel, "RMP2_QUAD_MINW": None if minw is None else str(minw)}
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return Engine(desc, 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(what, kernel="quad", **kw):
    import torch
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    s = _states()
    for solve in ("pinv", "auto"):
        _, desc = Cf.config3(solve)
        ref = O.step(desc, s["q"], s["qd"], s["goal"], **kw)
        spread = O.fp32_resolution(desc, s["q"], s["qd"], s["goal"], **kw)
        for minw in ((4, None) if kernel == "quad" else (None,)):
            eng = _engine(desc, kernel, minw)
            out = eng.step(torch.from_numpy(s["q"]), torch.from_numpy(s["qd"]), torch.from_numpy(s["goal"]),
                           obstacles=eng.obstacles(**{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in kw.items()}))
            torch.cuda.synchronize()
            name = eng.last_kernel()
            assert kernel in name, name
            got = out.cpu().numpy()
            verdict = O.accuracy_gate(got, ref, spread=spread)
            summary = O.gate_summary(verdict)
            print(f"{what} [{solve}, RMP2_QUAD_MINW={minw}]: {summary} [{name}]")
            assert np.isfinite(got).all(), f"{what}: non-finite output"
            assert verdict["ok"].all() and summary["rejected"] == 0, f"{what} [{solve}, {minw}]: {summary} ({name})"


@pytest.mark.gpu
def test_no_pair_in_range(hip_lib):
    """Zero trips in every wave: the loop is never entered."""
    _run("far table", spheres=_far_table())


@pytest.mark.gpu
def test_every_lane_on_every_trip(hip_lib):
    """32 spheres in range of one control point: eight trips of that quad with all four lanes at work."""
    from riemannian_motion_policies_amd import configs as Cf
    _, desc = Cf.config3()
    _run("hand table", spheres=_hand_table(_origins(desc, _states()["q"])))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [33, 40, 64])
def test_second_chunk(hip_lib, K):
    """Tables beyond 32 spheres: the trip loop is left and entered again for the second chunk (one sphere, eight, a full one)."""
    _run(f"{K} spheres", spheres=_sphere_table(K))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["mask", "list"])
def test_ragged_lists(hip_lib, form):
    """Per-robot lists as membership masks (the dense loop, masked) and with a repeated index (the list walk, 33 entries at
    the longest: a second chunk of one)."""
    off, idx = _ragged(form == "list")
    _run(f"ragged {form}", spheres=_sphere_table(32), csr_offset=off, csr_index=idx)


@pytest.mark.gpu
def test_capsule_table(hip_lib):
    """Capsules: the record of the next trip is fetched from global memory while the current one is evaluated."""
    _run("capsules", spheres=_capsule_table())


@pytest.mark.gpu
def test_hex_mapping(hip_lib):
    """The same sphere table through the 16-lane mapping (W == 16: pairs dealt by rank, two trips at the most)."""
    _run("32 spheres, hex", kernel="hex", spheres=_sphere_table(32))

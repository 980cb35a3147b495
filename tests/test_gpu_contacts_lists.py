"""Per-robot obstacle lists over a shared pool on the GPU (include/rmp2.h rmp2_dynamics_step_contacts_lists,
Engine.dynamics_step(contacts=pool, contact_lists=(csr_offset, csr_index))).

1. The stress catalogue of tests/contacts_scene.py as ONE launch per set of groups that share limits and tau_limit: the pool is
   the union of the groups' tables, a lane of group g lists g's slice (ascending), clear lanes list nothing.  Every lane equals,
   bit for bit (status word included), the same lane of the shared-table call on that group's table -- code this feature does not
   touch -- with contact_pair f K_g + k mapped to f K_pool + start_g + k.  Divergent trip counts, masked lanes and per-lane
   gathers in R = 130 (two waves and two lanes).
2. List lengths 0, 1, 7, 32 and 256 cycling over the 64 lanes of one wave, over a pool of 600 records (ascending, shuffled and
   with far-away filler): the fp64 reference on spheres[list] within the bounds of tests/test_contacts_host.py, unchanged, on the
   kept robots; each lane alone (R = 1) and the reversed fleet reproduce the lane's bits.
3. Four substeps on (1)'s fleets within K_STEP.
4. Invalid lists (an entry -1, an entry K) and a non-finite record owned by one robot, the pool being the interior of a larger
   tensor with a finite record on either side: that robot NaN with RMP2_CONTACT_LIST_INVALID, the others' bits untouched.
5. Refusals from Python and the C ABI.   6. A graph capture of the policy's step over ragged lists and the list contact step on
   the SAME csr tensors, replayed twice."""
import numpy as np
import pytest

import contacts_reference as CR
import contacts_scene as CS
import forward_dynamics_reference as FR
import test_contacts_host as S
import test_contacts_lists_host as L
from test_contacts_host import D_ACT, DT, K_STEP, STEP_SUBSTEPS
from test_gpu_contacts import _bits, _dev, _drive, _engine, _host, _step

pytestmark = pytest.mark.gpu

FLEETS = [("panda", FR.ACCEL), ("panda", FR.TORQUE), ("two_joint", FR.ACCEL), ("two_joint", FR.TORQUE)]
FLOATS = L.FLOATS


def _ints(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def _step_lists(eng, c, pool, off, idx, substeps=1, q=None, qd=None, u=None, d_act=D_ACT):
    """dict(q, qd, qdd, tau, stop, contact, lam, pair, status) of the list contact step on the case; pool: [K, 4] array or a
    device tensor."""
    import torch
    q, qd, u = _dev(c["q"] if q is None else q, c["qd"] if qd is None else qd, c["u"] if u is None else u)
    pool = pool if isinstance(pool, torch.Tensor) else _dev(np.asarray(pool, np.float32).reshape(-1, 4))[0]
    R = len(q)
    qdd, tau, stop, cont = torch.empty_like(q), torch.empty_like(q), torch.full_like(q, 7.0), torch.full_like(q, 7.0)
    lam = torch.full((R, 8), 7.0, device=q.device)
    pair = torch.full((R, 8), 5, dtype=torch.int32, device=q.device)
    status = torch.full((R,), -1, dtype=torch.int32, device=q.device)
    eng.dynamics_step(q, qd, u, DT, substeps=substeps, drive=_drive(c), tau_limit=c["lim"], qdd_out=qdd, tau_out=tau,
                      q_limits=c["limits"], stop_out=stop, status_out=status, contacts=pool, contact_lists=(_ints(off), _ints(idx)),
                      d_act=d_act, contact_out=cont, contact_lambda_out=lam, contact_pair_out=pair)
    return dict(q=_host(q), qd=_host(qd), qdd=_host(qdd), tau=_host(tau), stop=_host(stop), contact=_host(cont), lam=_host(lam),
                pair=_host(pair), status=_host(status).view(np.uint32))


def _rows(d, rows):
    return {k: v[rows] for k, v in d.items()}


def _same(a, b, what):
    for k in FLOATS:
        assert _bits(a[k], b[k]), (what, k)
    assert np.array_equal(a["pair"], b["pair"]) and np.array_equal(a["status"], b["status"]), what


@pytest.fixture(scope="module")
def groups(golden_dir):
    return CS.catalogue(golden_dir)


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(c):
        if c["name"] not in cache:
            cache[c["name"]] = _engine(c)
        return cache[c["name"]]
    return get


def _key(c):
    """What one launch shares beside the spheres: the box of limits and tau_limit."""
    lim = b"" if c["lim"] is None else np.asarray(c["lim"], np.float32).tobytes()
    return np.asarray(c["limits"][0], np.float32).tobytes() + np.asarray(c["limits"][1], np.float32).tobytes() + b"|" + lim


def fleet_launches(fleet):
    """(pool, start [groups], launches): the union of the groups' tables, where each group's slice starts, and per set of groups
    that share limits and tau_limit (groups, csr_offset, csr_index): lanes of those groups list their group's slice, ascending,
    every other lane nothing."""
    gs = fleet["groups"]
    start = np.concatenate([[0], np.cumsum([len(c["spheres"]) for c in gs])])
    pool = np.concatenate([c["spheres"] for c in gs])
    sets = {}
    for g, c in enumerate(gs):
        sets.setdefault(_key(c), []).append(g)
    launches = []
    for members in sets.values():
        lists = [np.arange(start[g], start[g + 1]) if g in members else np.zeros(0, np.int64) for g in fleet["lane_group"]]
        launches.append((members, *L.csr(lists)))
    return pool, start, launches


@pytest.fixture(scope="module")
def mixed(groups, engines):
    """Per robot and drive: (fleet, pool, start, [(groups of the launch, the list call's outputs)])."""
    out = {}
    for name, drive in FLEETS:
        fleet = CS.mixed_fleet(groups, name, drive)
        pool, start, launches = fleet_launches(fleet)
        outs = [(members, _step_lists(engines(fleet["groups"][members[0]]), CS.launch_case(fleet, members[0]), pool, off, idx))
                for members, off, idx in launches]
        out[(name, drive)] = (fleet, pool, start, outs)
    return out


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,drive", FLEETS)
def test_catalogue_in_one_launch_equals_the_shared_call_per_group_bit_for_bit(mixed, engines, name, drive):
    fleet, pool, start, outs = mixed[(name, drive)]
    assert len(fleet["q"]) == CS.MIXED_R == 130
    assert len(outs) < len(fleet["groups"]) and sum(len(m) for m, _ in outs) == len(fleet["groups"])      # (groups do share launches)
    clear = fleet["lane_group"] < 0
    contacts = 0
    for members, d in outs:
        lengths = {int(start[g + 1] - start[g]) for g in members} | {0}
        assert len(lengths) >= 2
        for g in members:
            c = fleet["groups"][g]
            want = _step(engines(c), CS.launch_case(fleet, g))
            lanes = np.nonzero(fleet["lane_group"] == g)[0]
            mapped = dict(want, pair=L.map_pairs(want["pair"], np.arange(start[g], start[g + 1]), len(pool)))
            _same(_rows(d, lanes), _rows(mapped, lanes), c["label"])
            _same(_rows(d, clear), _rows(want, clear), (c["label"], "clear lanes"))
            assert (d["pair"][clear] == -1).all()
            contacts += int((want["pair"][lanes] >= 0).sum())
    assert contacts >= 150


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 7, 32, 256)
K_POOL = 600


@pytest.fixture(scope="module")
def length_mix(golden_dir):
    """Per robot and drive (64 robots, a table of 16): (case, pool, lists per lane, [(rows, list, the group on spheres[list])])."""
    out = []
    rng = np.random.default_rng(1310)
    for c in S.contact_cases(golden_dir, seed=511, fleets=(("panda", 64), ("two_joint", 64)), n_spheres=16):
        pool, pos = L.embed(rng, c["spheres"], K_POOL)
        far = np.setdiff1d(np.arange(K_POOL), pos)
        touching = pos[np.unique(c["ref"]["pair"][c["ref"]["pair"] >= 0] % len(pos))]
        assert len(touching) >= 3
        by_len = {0: np.zeros(0, np.int64),
                  1: touching[:1],
                  7: rng.permutation(np.concatenate([touching[:3], rng.choice(far, 7 - len(touching[:3]), replace=False)])),
                  32: np.sort(np.concatenate([pos, rng.choice(far, 32 - len(pos), replace=False)])),
                  256: rng.permutation(np.concatenate([pos, rng.choice(far, 256 - len(pos), replace=False)]))}
        lists = [by_len[LENGTHS[r % 5]] for r in range(64)]
        groups = []
        for k, n in enumerate(LENGTHS):
            rows = np.arange(k, 64, 5)
            table = pool[by_len[n]] if n else L.filler(1)          # (the reference of an empty list: one sphere far away)
            groups.append((rows, by_len[n], CS._group(c, "lists", f"len{n}", c["q"][rows], c["qd"][rows], c["u"][rows], table, c["limits"], c["lim"])))
        out.append((c, pool, lists, groups))
    return out


def test_list_lengths_0_1_7_32_256_in_one_wave_against_the_reference(length_mix, engines):
    kept = 0
    for c, pool, lists, groups in length_mix:
        assert len(c["q"]) == 64 and [len(l) for l in lists[:5]] == list(LENGTHS)
        d = _step_lists(engines(c), c, pool, *L.csr(lists))
        for rows, lst, g in groups:
            got = _rows(d, rows)
            if len(lst) == 0:
                assert (got["pair"] == -1).all() and (got["lam"] == 0).all() and (got["contact"] == 0).all()
                CS.hard_invariants(g, got, g["label"])
                CS.check_kept(g, got, CS.kept(g), g["label"])
                continue
            kept += L.check_against_reference(g, got, lst, len(pool), g["label"])
        assert ((d["status"] & CR.CAPPED) == 0).all() and ((d["status"] & L.LIST_INVALID) == 0).all()
    print("kept", kept)
    assert kept >= 120


def test_each_lane_alone_and_the_reversed_fleet_have_the_lanes_bits(length_mix, engines):
    for c, pool, lists, _ in length_mix:
        eng = engines(c)
        d = _step_lists(eng, c, pool, *L.csr(lists))
        for r in range(10):          # (every length twice)
            sel = slice(r, r + 1)
            alone = _step_lists(eng, c, pool, *L.csr(lists[sel]), q=c["q"][sel], qd=c["qd"][sel], u=c["u"][sel])
            _same(alone, _rows(d, [r]), (c["name"], r))
        back = _step_lists(eng, c, pool, *L.csr(lists[::-1]), q=c["q"][::-1], qd=c["qd"][::-1], u=c["u"][::-1])
        _same(_rows(back, slice(None, None, -1)), d, (c["name"], "reversed"))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,drive", FLEETS)
def test_one_launch_over_four_substeps(mixed, engines, groups, name, drive):
    CS.with_steps(groups)
    fleet, pool, start, _ = mixed[(name, drive)]
    kept, worst = 0, 0.0
    for members, off, idx in fleet_launches(fleet)[2]:
        c0 = fleet["groups"][members[0]]
        d = _step_lists(engines(c0), CS.launch_case(fleet, members[0]), pool, off, idx, substeps=STEP_SUBSTEPS)
        for g in members:
            c = fleet["groups"][g]
            lanes = np.nonzero(fleet["lane_group"] == g)[0]
            rows = fleet["lane_robot"][lanes]
            got = _rows(d, lanes)
            CS.step_invariants(dict(c, q=c["q"][rows]), got, c["label"])
            keep = CS.kept_step(c)[rows]
            ref = c["ref_step"]
            bq, bqd = CR.step_brackets(ref, DT, STEP_SUBSTEPS)
            ratio = np.maximum(np.abs(got["q"] - ref["q"][rows]).max(1) / bq[rows], np.abs(got["qd"] - ref["qd"][rows]).max(1) / bqd[rows])
            assert (ratio[keep] <= K_STEP).all(), (c["label"], ratio.tolist())
            assert not (got["status"][keep] & CR.CAPPED).any(), c["label"]
            kept += int(keep.sum())
            worst = max(worst, float(ratio[keep].max(initial=0.0)))
    print(name, _drive(dict(drive=drive)), "worst step ratio", worst, "kept", kept)
    assert kept >= 70


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------

def test_invalid_and_non_finite_lists_poison_only_their_robot(length_mix, engines):
    import torch
    for c, _, _, _ in length_mix:
        eng = engines(c)
        K = len(c["spheres"])
        R = 65
        q, qd, u = (np.concatenate([c[k], c[k][:1]]) for k in ("q", "qd", "u"))
        # the pool is the interior of a larger tensor; the records beside it are finite, far away and distinguishable
        big = _dev(np.concatenate([L.filler(1, 900), c["spheres"], L.filler(1, 901)]))[0]
        pool = big[1:K + 1]
        assert pool.data_ptr() == big.data_ptr() + 16 and pool.is_contiguous()
        lists = [np.arange(K) for _ in range(R)]
        good = _step_lists(eng, c, pool, *L.csr(lists), q=q, qd=qd, u=u)
        assert np.isfinite(good["qd"]).all() and (good["pair"] >= 0).any()
        bad = [3, 64]
        others = np.setdiff1d(np.arange(R), bad)
        for entries in ((-1, K), (K, -1)):
            broken = [l.copy() for l in lists]
            broken[3][K // 2], broken[64][0] = entries
            d = _step_lists(eng, c, pool, *L.csr(broken), q=q, qd=qd, u=u)
            L.all_nan(d, bad, entries)
            assert (d["status"][bad] == L.LIST_INVALID).all(), d["status"][bad]
            _same(_rows(d, others), _rows(good, others), entries)
        # a non-finite record that robots 3 and 64 alone list
        big2 = _dev(np.concatenate([L.filler(1, 900), c["spheres"], L.filler(2, 901)]))[0]
        pool2 = big2[1:K + 2]
        owners = [l.copy() for l in lists]
        owners[3] = np.arange(K + 1)
        owners[64] = np.array([K])
        good2 = _step_lists(eng, c, pool2, *L.csr(owners), q=q, qd=qd, u=u)
        assert np.isfinite(good2["qd"]).all()
        big2[K + 1, 1] = float("inf")
        d = _step_lists(eng, c, pool2, *L.csr(owners), q=q, qd=qd, u=u)
        L.all_nan(d, bad, "non-finite record")
        _same(_rows(d, others), _rows(good2, others), "non-finite record")
        torch.cuda.synchronize()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------

def test_refusals(length_mix):
    import ctypes as C
    import torch
    from riemannian_motion_policies_amd import _native, engine as E
    c = next(c for c, _, _, _ in length_mix if c["name"] == "panda")
    eng = _engine(c)
    q, qd, u = (torch.zeros((4, 9), device="cuda") for _ in range(3))
    sph = torch.zeros((3, 4), device="cuda")
    off, idx = _ints(np.zeros(5)), _ints(np.zeros(1))
    with pytest.raises(ValueError, match="contact_lists needs contacts"):
        eng.dynamics_step(q, qd, u, DT, contact_lists=(off, idx))
    with pytest.raises(ValueError, match="pair"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, contact_lists=off, d_act=0.01)
    with pytest.raises(ValueError, match="csr_offset must be"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, contact_lists=(off.long(), idx), d_act=0.01)
    with pytest.raises(ValueError, match="csr_index must be"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, contact_lists=(off, idx.float()), d_act=0.01)
    with pytest.raises(ValueError, match="csr_offset must be"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, contact_lists=(off.cpu(), idx), d_act=0.01)
    with pytest.raises(ValueError, match="csr_index must be"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, contact_lists=(off, idx.cpu()), d_act=0.01)
    with pytest.raises(ValueError, match="csr_offset must be"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, contact_lists=(_ints(np.zeros(4)), idx), d_act=0.01)
    with pytest.raises(ValueError, match="csr_index must be"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, contact_lists=(off, idx.reshape(1, 1)), d_act=0.01)
    with pytest.raises(_native.Rmp2Error, match="d_act"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, contact_lists=(off, idx), d_act=-1.0)
    with pytest.raises(_native.Rmp2Error, match="substeps"):
        eng.dynamics_step(q, qd, u, DT, substeps=0, contacts=sph, contact_lists=(off, idx), d_act=0.01)
    # a pool of more than 256 records is fine with lists, and still refused without
    big = torch.zeros((300, 4), device="cuda")
    big[:, 0] = 50.0
    eng.dynamics_step(q, qd, u, DT, contacts=big, contact_lists=(off, idx), d_act=0.01)
    with pytest.raises(_native.Rmp2Error, match="K > 256"):
        eng.dynamics_step(q, qd, u, DT, contacts=big, d_act=0.01)
    # every list empty and csr_index a tensor of no elements: accepted (the engine passes a readable stand-in made beforehand)
    assert eng._empty_index is not None
    eng.dynamics_step(q, qd, u, DT, contacts=big, contact_lists=(off, _ints(np.zeros(0))), d_act=0.01)
    q.zero_(), qd.zero_()
    # the C ABI: a pool beyond RMP2_MAX_CONTACT_POOL (refused on the host: the small buffer is never read), K < 0, null lists,
    # a misaligned pool
    lib, h = eng._lib, eng._h
    s = torch.cuda.current_stream().cuda_stream

    def call(pool_ptr, K, off_ptr, idx_ptr):
        return lib.rmp2_dynamics_step_contacts_lists(h, q.data_ptr(), qd.data_ptr(), u.data_ptr(), 1, None, None, None, pool_ptr, K,
                                                     off_ptr, idx_ptr, C.c_float(0.01), C.c_float(DT), 1, None, None, None, None,
                                                     None, None, None, 4, s)
    assert call(sph.data_ptr(), E.MAX_CONTACT_POOL + 1, off.data_ptr(), idx.data_ptr()) != 0
    assert "K > 16777216" in lib.rmp2_last_error(h).decode()
    assert call(sph.data_ptr(), -1, off.data_ptr(), idx.data_ptr()) != 0
    assert call(sph.data_ptr(), 3, None, idx.data_ptr()) != 0 and "null array" in lib.rmp2_last_error(h).decode()
    assert call(sph.data_ptr(), 3, off.data_ptr(), None) != 0
    assert call(None, 3, off.data_ptr(), idx.data_ptr()) != 0
    assert call(sph.data_ptr() + 4, 2, off.data_ptr(), idx.data_ptr()) != 0 and "aligned" in lib.rmp2_last_error(h).decode()
    assert call(None, 0, off.data_ptr(), idx.data_ptr()) == 0            # K == 0 with empty lists is the stops' step
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q).all())
    bare = _engine(c, capsules=False)
    with pytest.raises(_native.Rmp2Error, match="rmp2_set_contact_capsules"):
        bare.dynamics_step(q, qd, u, DT, contacts=sph, contact_lists=(off, idx), d_act=0.01)


def test_sixteen_dof_robot_is_refused_as_unsupported(tmp_path):
    import torch
    import dynamics_reference as DR
    from riemannian_motion_policies_amd import _native, descriptor as D, urdf as U
    from riemannian_motion_policies_amd.engine import Engine
    path = str(tmp_path / "dof16.urdf")
    order = DR.random_urdf(np.random.default_rng(3), path, 16, n_dof=16, chain=True, massless=0.0, prismatic=0.0, fixed=0.0)
    t = U.compile_urdf(path, order)
    eng = Engine(D.build_desc(t, []), 0)
    eng.set_inertials(U.inertial_table(t, U.read_inertials(path)))
    caps = np.zeros((t.n_frames, 8), np.float32)
    caps[:, 3] = 0.05
    eng.set_contact_capsules(caps)
    q, qd, u = (torch.zeros((2, 16), device="cuda") for _ in range(3))
    with pytest.raises(_native.Rmp2Error, match="more than 9 dofs") as e:
        eng.dynamics_step(q, qd, u, DT, contacts=torch.zeros((1, 4), device="cuda"), contact_lists=(_ints(np.zeros(3)), _ints(np.zeros(1))),
                          d_act=0.01)
    assert e.value.code == _native.ERR_UNSUPPORTED


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------

def test_graph_capture_of_ragged_policy_step_and_list_contact_step_replays_twice(golden_dir):
    """The experiment loop's body with every robot in its own clutter -- the policy's step over ragged lists (the fused route),
    then the plant's step with stops and contacts over the SAME csr_offset / csr_index tensors and the same pool -- captured once
    and replayed twice from the same state: the bytes of the eager run."""
    import torch
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    from riemannian_motion_policies_amd.engine import Engine
    from test_inverse_dynamics_host import reference_robots
    _, desc = Cf.config3()
    eng = Engine(desc, 0)
    t = U.panda_table()
    eng.set_inertials(next(i for n, _, i in reference_robots(golden_dir) if n == "panda"))
    eng.set_contact_capsules(U.contact_capsules(U.PANDA_URDF, t))
    R = 512
    s = Cf.sample_panda_states(np.random.default_rng(40), R)
    rng = np.random.default_rng(42)
    base = Cf.sample_spheres(np.random.default_rng(41))[:, :4]
    pool_np = np.concatenate([base + np.concatenate([rng.normal(0.0, 0.02, 3), [0.0]]).astype(np.float32) for _ in range(8)]).astype(np.float32)
    lists = [np.sort(rng.choice(len(pool_np), int(rng.integers(0, 25)), replace=False)) for _ in range(R)]
    off, idx = (_ints(x) for x in L.csr(lists))
    pool = torch.from_numpy(pool_np).cuda().contiguous()
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    q0, qd0 = q.clone(), qd.clone()
    obs = eng.obstacles(spheres=pool, csr_offset=off, csr_index=idx)
    assert obs._keep[1].data_ptr() == off.data_ptr() and obs._keep[2].data_ptr() == idx.data_ptr()      # the same tensors, no copy
    lim = torch.from_numpy(U.read_effort_limits(U.PANDA_URDF, U.PANDA_ORDER)).cuda()
    lo, hi = (torch.from_numpy(x).cuda() for x in U.read_joint_limits(U.PANDA_URDF, U.PANDA_ORDER))
    side = torch.cuda.Stream()
    launch, qdd = eng.bind(q, qd, goal, obstacles=obs, stream=side.cuda_stream)
    outs = [torch.empty_like(q) for _ in range(4)]
    lam = torch.empty((R, 8), device="cuda")
    pair = torch.empty((R, 8), dtype=torch.int32, device="cuda")
    status = torch.empty(R, dtype=torch.int32, device="cuda")

    def chain():
        launch()
        eng.dynamics_step(q, qd, qdd, DT, substeps=3, tau_limit=lim, qdd_out=outs[0], tau_out=outs[1], q_limits=(lo, hi),
                          stop_out=outs[2], status_out=status, contacts=pool, contact_lists=(off, idx), d_act=0.05,
                          contact_out=outs[3], contact_lambda_out=lam, contact_pair_out=pair)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        chain()
    side.synchronize()
    everything = (q, qd, qdd, *outs, lam, pair, status)
    eager = [x.clone() for x in everything]
    assert not torch.equal(q, q0) and bool(torch.isfinite(q).all())
    assert not bool((status & L.LIST_INVALID).any())
    g = torch.cuda.CUDAGraph()
    q.copy_(q0)
    qd.copy_(qd0)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):   # one stream, no parallel branches
        chain()
    for _ in range(2):
        for x in (*outs, lam, pair, status):
            x.zero_()
        q.copy_(q0)
        qd.copy_(qd0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(everything, eager):
            assert torch.equal(a, b)

"""Host side of the quad mapping's structured identity-leaf loop (csrc/rmp2_device.h IdLeafRec, filled by the program compiler
in csrc/rmp2_hip.hip): rmp2_identity_records shows the records a descriptor compiles to, without a GPU.  Checked here: which
sets get records at all, their order, their fixed layout, and that the three derived values carry the bits of the fp32
expressions the general loop evaluates on the device (P[0] - P[1], P[1] - 1e-6f, P[0] + P[4], each rounded once)."""
import ctypes as C

import numpy as np

from riemannian_motion_policies_amd import configs as Cf, descriptor as D
from riemannian_motion_policies_amd.urdf import panda_table

WORDS = 32  # per record: kind | three derived values | P[0..11] | vec_a[0..15]


def _records(lib, desc, capacity=D.MAX_LEAVES):
    buf = np.full((max(capacity, 1), WORDS), 0x7FC00000, dtype=np.uint32)
    n = lib.rmp2_identity_records(C.byref(desc), buf.ctypes.data_as(C.c_void_p), capacity)
    return n, buf


def _lib(hip_lib):
    lib = C.CDLL(hip_lib)
    lib.rmp2_identity_records.argtypes = [C.POINTER(D.Desc), C.c_void_p, C.c_int32]
    lib.rmp2_identity_records.restype = C.c_int
    return lib


def test_config3_compiles_to_three_records_in_execution_order(hip_lib):
    lib = _lib(hip_lib)
    for solve in ("auto", "pinv"):
        _, desc = Cf.config3(solve)
        n, buf = _records(lib, desc)
        assert n == 3
        want = [(D.LEAF_JOINT_VELOCITY_CAP, Cf.JOINT_VELOCITY_CAP_PARAMS, None), (D.LEAF_JOINT_DAMPING, Cf.JOINT_DAMPING_PARAMS, None),
                (D.LEAF_CSPACE_BIASING, Cf.CSPACE_BIASING_PARAMS, Cf.CSPACE_BIASING_GOAL)]
        for rec, (kind, params, va) in zip(buf, want):
            assert int(rec[0].view(np.int32)) == kind
            P = np.zeros(D.MAX_PARAMS, dtype=np.float32)
            P[: len(params)] = np.asarray(params, dtype=np.float32)
            assert np.array_equal(rec[4:16], P.view(np.uint32))
            # the derived values: the fp32 expressions of the device code, bit for bit
            derived = np.array([P[0] - P[1], P[1] - np.float32(1e-6), P[0] + P[4]], dtype=np.float32)
            assert np.array_equal(rec[1:4], derived.view(np.uint32)), (kind, rec[1:4].view(np.float32), derived)
            vec = np.zeros(16, dtype=np.float32)
            if va is not None:
                vec[: len(va)] = np.asarray(va, dtype=np.float32)
            assert np.array_equal(rec[16:32], vec.view(np.uint32))
        assert (buf[3:] == 0x7FC00000).all()  # nothing written behind the last record


def test_derived_values_are_rounded_once_in_fp32(hip_lib):
    """Parameters whose fp32 difference / sum differs from the rounded fp64 one would expose a host that computes in double."""
    lib = _lib(hip_lib)
    t = panda_table()
    rng = np.random.default_rng(3)
    for _ in range(20):
        p = rng.uniform(0.01, 3.0, 5).astype(np.float32) * np.float32(1.0000001)
        specs = [D.LeafSpec(D.LEAF_JOINT_VELOCITY_CAP, D.TASKMAP_IDENTITY, -1, [float(x) for x in p[:4]]),
                 D.LeafSpec(D.LEAF_CSPACE_BIASING, D.TASKMAP_IDENTITY, -1, [float(x) for x in p], vec_a=rng.uniform(-1, 1, 9))]
        n, buf = _records(lib, D.build_desc(t, specs))
        assert n == 2
        for rec in buf[:2]:
            P = rec[4:16].view(np.float32)
            derived = np.array([P[0] - P[1], P[1] - np.float32(1e-6), P[0] + P[4]], dtype=np.float32)
            assert np.array_equal(rec[1:4], derived.view(np.uint32))


def test_a_dense_identity_leaf_means_no_records(hip_lib):
    lib = _lib(hip_lib)
    for build in (Cf.config1, Cf.config2, Cf.exp04_panda_identity_target):
        _, desc = build()
        n, buf = _records(lib, desc)
        assert n == 0 and (buf == 0x7FC00000).all(), build.__name__
    t = panda_table()
    damping = D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS)
    limits = D.LeafSpec(D.LEAF_JOINT_LIMIT_AVOIDANCE, D.TASKMAP_IDENTITY, -1, Cf.JOINT_LIMIT_PARAMS, vec_a=Cf.PANDA_Q_LOW, vec_b=Cf.PANDA_Q_HIGH)
    for specs in ([limits, damping], [damping, limits]):
        assert _records(lib, D.build_desc(t, specs))[0] == 0
    assert _records(lib, D.build_desc(t, [damping]))[0] == 1


def test_capacity_and_arguments(hip_lib):
    lib = _lib(hip_lib)
    _, desc = Cf.config3()
    n, buf = _records(lib, desc, capacity=2)  # the count is returned in full, only `capacity` records are written
    assert n == 3 and int(buf[1][0].view(np.int32)) == D.LEAF_JOINT_DAMPING
    assert lib.rmp2_identity_records(C.byref(desc), None, 0) == 3
    assert lib.rmp2_identity_records(None, None, 0) == -1
    assert lib.rmp2_identity_records(C.byref(desc), None, 1) == -1

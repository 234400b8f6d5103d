"""CPU: the host side of the clocks' op path — every new header function
(include/crdts_hip.h "Batched op path of the clocks and counters") has a ctypes
binding and is exported; the host VClock mirror's truncate / subtract /
intersection reproduce the reference's subtract KATs (test/vclock.rs:54-78, in
tests/golden/kat_vclock_counters.json) and agree with the oracle restatement
(oracle/crdts_ref.py) on random small clocks; ClockOps packs the arrays
crdt_clock_ops describes; and argument checks come before any device work."""
import ctypes as C
import json
import os
import random

import numpy as np

import crdts_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

NEW = ["crdt_vclock_dense_apply", "crdt_gcounter_apply", "crdt_pncounter_apply", "crdt_vclock_dense_truncate",
       "crdt_vclock_dense_subtract", "crdt_vclock_dense_intersection", "crdt_gcounter_value", "crdt_pncounter_value",
       "crdt_vclock_dense_get", "crdt_vclock_csr_truncate", "crdt_vclock_csr_subtract", "crdt_vclock_csr_intersection",
       "crdt_vclock_csr_apply", "crdt_gcounter_csr_apply", "crdt_gcounter_csr_value", "crdt_vclock_csr_get"]


def _kats():
    return json.load(open(os.path.join(GOLDEN, "kat_vclock_counters.json")))


def test_every_new_function_is_declared_bound_and_exported():
    import crdts_hip
    from crdts_hip._lib import lib

    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "crdts_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in crdts_hip.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name  # a declared signature, not ctypes' default
    for m in ("dense_apply", "dense_truncate", "dense_subtract", "dense_intersection", "gcounter_value",
              "pncounter_value", "dense_get", "clock_csr_apply", "clock_csr_truncate", "clock_csr_subtract",
              "clock_csr_intersection", "clock_csr_value", "clock_csr_get", "pncounter_csr_apply",
              "pncounter_csr_value"):
        assert callable(getattr(crdts_hip.Engine, m)), m


def test_mirror_reproduces_the_subtract_kats():
    import crdts_hip

    kats = [k for k in _kats()["vclock_binop"] if k["op"] == "subtract"]
    assert len(kats) == 3  # test_subtract and the two property instances
    for k in kats:
        a, b = crdts_hip.VClock(k["a"]), crdts_hip.VClock(k["b"])
        a.subtract(b)
        assert sorted(a.dots.items()) == [tuple(x) for x in k["expect"]], k["name"]
    # the properties the instances come from (test/vclock.rs:46-66), on the mirror
    a = crdts_hip.VClock([(3, 2), (9, 1)])
    t = crdts_hip.VClock([(3, 2), (9, 1)])
    t.truncate(a)
    assert t.dots == a.dots  # truncate by self is the identity
    assert a.intersection(a).dots == a.dots


def test_mirror_agrees_with_the_oracle_restatement_on_random_clocks():
    import crdts_hip

    rng = random.Random(20)

    def clock():
        return [(rng.randrange(6), rng.choice([0, 1, 1, 2, 3, (1 << 64) - 1])) for _ in range(rng.randrange(7))]

    for _ in range(400):
        pa, pb = clock(), clock()
        for op in ("truncate", "subtract", "intersection"):
            m, mo = crdts_hip.VClock(pa), crdts_hip.VClock(pb)
            r, ro = crdts_ref.VClock(pa), crdts_ref.VClock(pb)
            assert m.dots == r.dots
            got, exp = getattr(m, op)(mo), getattr(r, op)(ro)
            if op == "intersection":
                assert got.dots == exp.dots and m.dots == r.dots  # self is untouched
            else:
                assert got is None and m.dots == r.dots
            assert mo.dots == ro.dots
            assert all(c > 0 for c in m.dots.values())


def test_clock_ops_from_lists_builds_the_documented_arrays():
    import crdts_hip

    per_obj = [[(3, 7), (0, 1)], [], [(5, 0)], [(2, (1 << 64) - 1), (2, 4), ((1 << 32) - 1, 9)]]
    ops = crdts_hip.ClockOps.from_lists(per_obj, device=None)
    assert (ops.n_obj, ops.n_ops) == (4, 6)
    ends, act, ctr, dr = ops.host
    assert ends.dtype == np.uint64 and ends.tolist() == [2, 2, 3, 6]
    assert act.dtype == np.uint32 and act.tolist() == [3, 0, 5, 2, 2, (1 << 32) - 1]
    assert ctr.dtype == np.uint64 and ctr.tolist() == [7, 1, 0, (1 << 64) - 1, 4, 9]
    assert dr is None and ops.t[3] is None
    # the tensors hold the same bits, in the widths of crdt_clock_ops
    assert ops.t[0].numpy().view(np.uint64).tolist() == ends.tolist()
    assert ops.t[1].numpy().view(np.uint32).tolist() == act.tolist()
    assert ops.t[2].numpy().view(np.uint64).tolist() == ctr.tolist()
    c = ops.cops()
    assert c.n_ops == 6 and c.dir is None and c.obj_end == ops.t[0].data_ptr() and c.actor == ops.t[1].data_ptr()
    # PNCounter ops carry Dir; a query batch is bare actors
    pn = crdts_hip.ClockOps.from_lists([[(1, 2, 0), (1, 3, 1)], [(0, 1, 1)]], with_dir=True, device=None)
    assert pn.host[3].dtype == np.uint32 and pn.host[3].tolist() == [0, 1, 1] and pn.host[0].tolist() == [2, 3]
    assert pn.cops().dir == pn.t[3].data_ptr()
    q = crdts_hip.ClockOps.from_lists([[4, 1], [], [0]], device=None)
    assert q.host[1].tolist() == [4, 1, 0] and q.host[0].tolist() == [2, 2, 3] and q.host[2].tolist() == [0, 0, 0]
    empty = crdts_hip.ClockOps.from_lists([[], []], device=None)
    assert (empty.n_obj, empty.n_ops) == (2, 0) and empty.cops().actor is None


def test_argument_checks_come_before_any_device_work():
    """No context exists here, so anything but CRDT_EINVAL would mean the call
    got past its checks (null ctx is the first of them)."""
    from crdts_hip._lib import CRDT_EINVAL, ClockCsr, ClockCsrOut, ClockOpsC, lib

    ops, s, w = ClockOpsC(), ClockCsr(), ClockCsrOut()
    for name in ("crdt_vclock_dense_apply", "crdt_gcounter_apply", "crdt_pncounter_apply"):
        assert getattr(lib, name)(None, None, C.byref(ops), 0, 4, None) == CRDT_EINVAL, name
    for name in ("crdt_vclock_dense_truncate", "crdt_vclock_dense_subtract", "crdt_vclock_dense_intersection",
                 "crdt_gcounter_value", "crdt_pncounter_value"):
        assert getattr(lib, name)(None, None, None, 0, 4, None) == CRDT_EINVAL, name
    assert lib.crdt_vclock_dense_get(None, None, C.byref(ops), None, 0, 4, None) == CRDT_EINVAL
    for name in ("crdt_vclock_csr_truncate", "crdt_vclock_csr_subtract", "crdt_vclock_csr_intersection"):
        assert getattr(lib, name)(None, C.byref(s), C.byref(s), C.byref(w), None) == CRDT_EINVAL, name
    for name in ("crdt_vclock_csr_apply", "crdt_gcounter_csr_apply"):
        assert getattr(lib, name)(None, C.byref(s), C.byref(ops), C.byref(w), None) == CRDT_EINVAL, name
    assert lib.crdt_gcounter_csr_value(None, C.byref(s), None, None) == CRDT_EINVAL
    assert lib.crdt_vclock_csr_get(None, C.byref(s), C.byref(ops), None, None) == CRDT_EINVAL

"""The yardstick of the batched nested-map op path (crdt_map_map_apply): the
generated op streams (tests/nested_opgen.py) reach every situation of
Map::apply on Map<u64, Map<u64, MVReg>> (src/map.rs:160-190, apply_rm
:336-350, apply_deferred :325-333, Map::truncate :131-158) that the kernel has
to get right, crdts_hip.MapMapOps packs every op kind as crdt_map_map_ops
specifies, and the hand-built cases the generator does not reach
(tests/golden/nested_apply_cases.json) hold on the Python restatement. No GPU
needed; the C ABI's argument check is called without a device."""
import numpy as np
import pytest

import map_kat_runner as mkr
import nested_opgen as ng

A = 16


def test_generated_streams_cover_the_op_path():
    batch = ng.gen_batch(0x0A55, 2000, A)
    st = ng.batch_stats(batch)
    print(st)
    assert st["ups"] > 5000 and st["dup"] > 300       # duplicate-dot skips
    assert st["up_rm"] > 200 and st["up_nop"] > 500 and st["rm"] > 500 and st["up_up"] > 2000
    assert st["end_outer_def"] > 200 and st["end_inner_def"] > 50
    assert st["trunc_def"] > 50                        # inner truncations of a map that holds deferred removes
    # the seven capacities the states need at any step (ng.sizes' order): within the tests' out capacities
    ko, do, so, ki, mi, di, si = st["peak"]
    assert (ko, do, so) <= ng.OUT_CAPS and all(x <= c for x, c in zip((ko, do, so), ng.OUT_CAPS))
    assert all(x <= c for x, c in zip((ki, mi, di, si), ng.OUT_INNER))
    # and the start states within the in capacities (packing asserts it too)
    for start, _ in batch[:200]:
        z = ng.sizes(start)
        assert all(x <= c for x, c in zip(z[:3], ng.IN_CAPS)) and all(x <= c for x, c in zip(z[3:], ng.IN_INNER))


def test_map_map_ops_packing():
    """MapMapOps.arrays_from_lists: every kind, its fields and its clock pairs."""
    import crdts_hip

    put = {"up": {"dot": [3, 7], "key": 11, "op": {"up": {"dot": [4, 9], "key": 12,
                                                          "op": {"put": {"clock": [[1, 2], [3, 7]], "val": 99}}}}}}
    irm = {"up": {"dot": [5, 1], "key": 21, "op": {"rm": {"clock": [[0, 4]], "key": 22}}}}
    inop = {"up": {"dot": [6, 2], "key": 31, "op": "nop"}}
    orm = {"rm": {"clock": [[2, 5], [6, 1], [7, 3]], "key": 41}}
    arrs = dict(zip(ng.OPS_FIELDS, crdts_hip.MapMapOps.arrays_from_lists([[put, "nop", irm], [], [inop, orm]])))
    assert tuple(crdts_hip.MapMapOps.FIELDS) == ng.OPS_FIELDS
    M = crdts_hip.MapMapOps
    assert (M.NOP, M.RM, M.UP_UP, M.UP_RM, M.UP_NOP) == (0, 1, 2, 3, 4)
    exp = dict(obj_end=[3, 3, 5], kind=[2, 0, 3, 4, 1], key=[11, 0, 21, 31, 41], actor=[3, 0, 5, 6, 0],
               counter=[7, 0, 1, 2, 0], key2=[12, 0, 22, 0, 0], actor2=[4, 0, 0, 0, 0], counter2=[9, 0, 0, 0, 0],
               val=[99, 0, 0, 0, 0], clk_end=[2, 2, 3, 3, 6], clk_act=[1, 3, 0, 2, 6, 7], clk_ctr=[2, 7, 4, 5, 1, 3])
    for f in ng.OPS_FIELDS:
        assert arrs[f].tolist() == exp[f], f
        assert arrs[f].dtype == (np.uint32 if f in ("kind", "actor", "actor2", "clk_act") else np.uint64), f
    with pytest.raises(ValueError):
        crdts_hip.MapMapOps.arrays_from_lists([[{"put": 1}]])
    # the C struct mirrors the header's field order
    from crdts_hip._lib import MapMapOpsC

    assert [f for f, _ in MapMapOpsC._fields_] == list(ng.OPS_FIELDS) + ["n_ops", "n_clk"]


def test_map_map_apply_rejects_bad_arguments_without_a_device():
    """CRDT_EINVAL comes before any device work."""
    import ctypes as C

    import crdts_hip
    from crdts_hip._lib import MapMapOpsC, lib

    S = crdts_hip.MapMapSlab.alloc(1, A, *ng.IN_CAPS, ng.IN_INNER)
    R = crdts_hip.MapMapSlab.alloc(1, A, *ng.OUT_CAPS, ng.OUT_INNER)
    s, r, o = S.cstruct(), R.cstruct(), MapMapOpsC()
    assert lib.crdt_map_map_apply(None, C.byref(s), C.byref(o), C.byref(r), 1, A, None, 0, None) == crdts_hip.CRDT_EINVAL
    assert lib.crdt_map_map_apply_scratch_bytes(None, 1, A) == 0
    need = lib.crdt_map_map_apply_scratch_bytes(C.byref(r), 3, A)
    inner_row = 8 * (A + 8 + 8 * A + 8 * 8 * A + 8 * 8 + 8 * A + 8 * 8) + 4 * (1 + 8 + 1 + 8)
    assert need >= 3 * 8 * (inner_row + 8 + 4)


CASES = ng.load_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_built_case_on_the_restatement(case):
    start = ng.case_start(case)
    ng.check_case_state(start, case["pre_checks"], case["name"] + " pre")
    end = ng.replay(start, case["ops"])
    ng.check_case_state(end, case["checks"], case["name"])
    if "alt_ops" in case:
        assert ng.replay(start, case["alt_ops"]) == end
    # the states fit the capacities the GPU test uses
    for m in (start, end):
        z = ng.sizes(m)
        assert all(x <= c for x, c in zip(z[:3], ng.IN_CAPS)) and all(x <= c for x, c in zip(z[3:], ng.IN_INNER))


def test_generator_does_not_reach_the_collapse():
    """Why case (a) is hand-built: no generated truncation makes two inner
    deferred clocks equal."""
    st = {}
    with ng.count_truncations(st):
        for start, ops in ng.gen_batch(0x0A55, 2000, A)[:500]:
            ng.replay(start, ops)
    assert st["trunc"] > 500 and st["collapse"] == 0
    st = {}
    case = next(c for c in CASES if c["name"] == "a_collapse")
    with ng.count_truncations(st):
        ng.replay(ng.case_start(case), case["ops"])
    assert st["collapse"] == 1


def test_nested_kats_apply_steps_are_literal_ops():
    """Every apply step of the seven nested KATs has the JSON form MapMapOps packs."""
    import crdts_hip

    cases = mkr.load_cases(nested=True)
    assert len(cases) == 7
    seen = []

    class Rec(ng.LiteralOpsBackend):
        def apply_raw(self, m, op):
            seen.append(op)
            super().apply_raw(m, op)

    for c in cases:
        mkr.run_case(c, Rec())
    assert len(seen) == sum(st[0] == "apply" for c in cases for st in c["steps"])
    kinds = crdts_hip.MapMapOps.arrays_from_lists([seen])[1]
    assert set(kinds.tolist()) >= {crdts_hip.MapMapOps.UP_UP, crdts_hip.MapMapOps.RM}

"""The yardstick of the batched Map<u64, MVReg>::apply (crdt_map_mvreg_apply):
on generated op streams (tests/map_opgen.py) the Python restatement
(oracle/crdts_ref.py) and the C++ oracle's Map handles agree after every op,
and the streams reach every situation of Map::apply (src/map.rs:160-190,
apply_rm :336-350, apply_deferred :325-333) that the kernel has to get right.
No GPU needed; the C ABI's argument check is called without a device."""
import ctypes as C

import map_opgen
import map_slab
from map_slab import crdts_ref

A = 8
CAPS = dict(kcap=8, mcap=8, dcap=8, scap=8)


def _view(h):
    return map_slab.mvreg_map_from_row(h.slab(A, CAPS), 0)


def test_python_and_oracle_agree_after_every_op_and_cover(oracle):
    batch = map_opgen.gen_batch(0xA991, 300, A)
    cov = dict(dup_dot=0, rm_deferred=0, deferred_retired_by_up=0, entry_removed_by_rm=0, deferred_set_grown=0,
               fresh_entry_removed_in_up=0, concurrent_values=0, empty_put_clock=0, ends_with_deferred=0)
    big = dict(keys=0, vals=0, defs=0, set=0, ops=0)
    for pre, ops in batch:
        py, h = crdts_ref.Map(crdts_ref.MVReg), oracle.OracleMap("mvreg")
        for op in pre:
            map_opgen.apply_op(py, op)
            map_opgen.apply_op_oracle(h, op)
        before = _view(h)
        assert before == py
        concurrent = False
        for op in ops:
            map_opgen.apply_op(py, op)
            map_opgen.apply_op_oracle(h, op)
            after = _view(h)  # the coverage below is counted on the oracle's states alone
            assert after == py, op
            if op[0] == "up":
                _, actor, counter, key, pairs, _ = op
                dup = before.clock.get(actor) >= counter
                cov["dup_dot"] += dup
                cov["empty_put_clock"] += not pairs
                if not dup:
                    cov["deferred_retired_by_up"] += any(c not in after.deferred for c in before.deferred)
                    cov["fresh_entry_removed_in_up"] += key not in before.entries and key not in after.entries
            else:
                _, key, pairs = op
                clock = crdts_ref.VClock(pairs)
                cov["rm_deferred"] += not (clock <= before.clock)
                cov["entry_removed_by_rm"] += key in before.entries and key not in after.entries
                cov["deferred_set_grown"] += clock in before.deferred and key not in before.deferred[clock] \
                    and key in after.deferred[clock]
            concurrent = concurrent or any(len(r.vals) >= 2 for _, r in after.entries.values())
            big["keys"] = max(big["keys"], len(after.entries))
            big["vals"] = max([big["vals"]] + [len(r.vals) for _, r in after.entries.values()])
            big["defs"] = max(big["defs"], len(after.deferred))
            big["set"] = max([big["set"]] + [len(s) for s in after.deferred.values()])
            before = after
        cov["concurrent_values"] += concurrent
        cov["ends_with_deferred"] += bool(before.deferred)
        big["ops"] = max(big["ops"], len(ops))
    print("coverage", cov, "largest", big)
    assert all(v >= 5 for v in cov.values()), cov
    # the GPU tests size their slabs by this: inputs (4, 4, 4, 4), outputs (8, 8, 8, 8)
    assert big["keys"] <= 4 and big["vals"] <= 4 and big["defs"] <= 8 and big["set"] <= 4, big


def test_symbol_exported_and_null_ctx_is_einval():
    import crdts_hip
    from crdts_hip._lib import MapOpsC, lib

    assert "crdt_map_mvreg_apply" in crdts_hip.EXPORTS
    S = crdts_hip.MapSlab.alloc(1, A, 4, 4, 4, 4)
    R = crdts_hip.MapSlab.alloc(1, A, 8, 8, 8, 8)
    s, r, o = S.cstruct(), R.cstruct(), MapOpsC()
    assert lib.crdt_map_mvreg_apply(None, C.byref(s), C.byref(o), C.byref(r), 1, A, None) == crdts_hip.CRDT_EINVAL
    assert lib.crdt_map_mvreg_apply(None, None, None, None, 0, A, None) == crdts_hip.CRDT_EINVAL


def test_map_ops_arrays_from_lists():
    import crdts_hip

    ends, kind, key, act, ctr, val, cend, cact, cctr = crdts_hip.MapOps.arrays_from_lists(
        [[("up", 2, 5, 7, [(0, 1), (2, 5)], 99), ("nop",)], [], [("rm", 9, [(1, 3)])]])
    assert ends.tolist() == [2, 2, 3] and kind.tolist() == [2, 0, 1] and key.tolist() == [7, 0, 9]
    assert act.tolist() == [2, 0, 0] and ctr.tolist() == [5, 0, 0] and val.tolist() == [99, 0, 0]
    assert cend.tolist() == [2, 2, 3] and cact.tolist() == [0, 2, 1] and cctr.tolist() == [1, 5, 3]

"""The yardstick of the batched Map<u64, Orswot>::apply (crdt_map_orswot_apply):
on generated op streams (tests/map_orswot_opgen.py) the Python restatement
(oracle/crdts_ref.py) and the C++ oracle's Map handles agree after every op,
the streams reach every situation of Map::apply (src/map.rs:160-190, apply_rm
:336-350, apply_deferred :325-333) with Orswot values (src/orswot.rs:66-82,
:159-172, :195-211) that the kernel has to get right, and three hand-built
cases pin what the streams do not reach. No GPU needed; the C ABI's argument
check is called without a device."""
import ctypes as C

import map_orswot_opgen as og
import map_slab
from map_slab import crdts_ref

A = 8
CAPS = og.caps(16)


def _view(h):
    return map_slab.orswot_map_from_row(h.slab(A, CAPS), 0)


def test_python_and_oracle_agree_after_every_op_and_cover(oracle):
    batch = og.gen_batch(0x0A57, 300, A)
    cov = dict(dup_dot=0, map_rm_deferred=0, map_deferred_retired_by_up=0, entry_removed_by_rm=0,
               entry_kept_and_truncated_by_rm=0, truncate_drops_member=0, nested_rm_deferred=0,
               nested_deferred_retired=0, member_removed_by_nested_rm=0, up_rm_on_absent_key=0,
               fresh_entry_removed_in_up=0, ends_with_map_deferred=0, ends_with_nested_deferred=0)
    big = dict(keys=0, members=0, vdefs=0, vset=0, defs=0, set=0)
    big_in = dict(big)

    def sizes(into, m):
        into["keys"] = max(into["keys"], len(m.entries))
        into["defs"] = max(into["defs"], len(m.deferred))
        into["set"] = max([into["set"]] + [len(s) for s in m.deferred.values()])
        for _, o in m.entries.values():
            into["members"] = max(into["members"], len(o.entries))
            into["vdefs"] = max(into["vdefs"], len(o.deferred))
            into["vset"] = max([into["vset"]] + [len(s) for s in o.deferred.values()])

    for pre, ops in batch:
        py, h = og.new_map(), oracle.OracleMap("orswot")
        for op in pre:
            og.apply_op(py, op)
            og.apply_op_oracle(h, op)
        before = _view(h)
        assert before == py
        sizes(big_in, before)
        sizes(big, before)
        for op in ops:
            og.apply_op(py, op)
            og.apply_op_oracle(h, op)
            after = _view(h)  # the coverage below is counted on the oracle's states alone
            assert after == py, op
            b_set = before.entries[op[3 if op[0] != "rm" else 1]][1] if op[0] != "nop" and \
                op[3 if op[0] != "rm" else 1] in before.entries else None
            if op[0] in ("up_add", "up_rm"):
                actor, counter, key, member = op[1:5]
                dup = before.clock.get(actor) >= counter
                cov["dup_dot"] += dup
                if not dup:
                    cov["map_deferred_retired_by_up"] += any(c not in after.deferred for c in before.deferred)
                    cov["fresh_entry_removed_in_up"] += key not in before.entries and key not in after.entries
                    if op[0] == "up_rm":
                        clock = crdts_ref.VClock(op[5])
                        cov["up_rm_on_absent_key"] += b_set is None
                        cov["nested_rm_deferred"] += not (clock <= (b_set.clock if b_set else crdts_ref.VClock()))
                        cov["member_removed_by_nested_rm"] += b_set is not None and member in b_set.entries and \
                            key in after.entries and member not in after.entries[key][1].entries
            elif op[0] == "rm":
                _, key, pairs = op
                clock = crdts_ref.VClock(pairs)
                cov["map_rm_deferred"] += not (clock <= before.clock)
                cov["entry_removed_by_rm"] += key in before.entries and key not in after.entries
                kept = key in before.entries and key in after.entries and bool(pairs)
                cov["entry_kept_and_truncated_by_rm"] += kept
                cov["truncate_drops_member"] += kept and any(x not in after.entries[key][1].entries
                                                             for x in b_set.entries)
            cov["nested_deferred_retired"] += any(
                k in after.entries and any(c not in after.entries[k][1].deferred for c in o.deferred)
                for k, (_, o) in before.entries.items())
            sizes(big, after)
            before = after
        cov["ends_with_map_deferred"] += bool(before.deferred)
        cov["ends_with_nested_deferred"] += any(o.deferred for _, o in before.entries.values())
    print("coverage", cov, "largest", big, "largest input", big_in)
    assert all(v >= 5 for v in cov.values()), cov
    # the GPU tests size their slabs by this: inputs 4, outputs 8 on all six capacities
    assert all(v <= 4 for v in big_in.values()), big_in
    assert all(v <= 8 for v in big.values()), big


def _both(oracle, ops, m=None, order=crdts_ref.clock_order):
    """`ops` on the Python restatement and on the C++ handles, from map `m`
    (default: empty); they agree after every op. -> the final map."""
    py = og.new_map(order) if m is None else m.clone()
    if m is None:
        h = oracle.OracleMap("orswot")
    else:
        import crdts_hip

        S = crdts_hip.MapOrswotSlab.alloc(1, A, **CAPS)
        map_slab.orswot_map_to_row(m, S, 0, A)
        h = og.oracle_from_row(oracle, S, 0, A)
        assert _view(h) == m
    for op in ops:
        og.apply_op(py, op)
        og.apply_op_oracle(h, op)
        if order is crdts_ref.clock_order:
            assert _view(h) == py, op
    return py, _view(h)


def test_case_a_nested_rm_leaves_smaller_member_clock(oracle):
    py, _ = _both(oracle, og.CASE_A)
    assert py.entries[7][1].entries == {1: crdts_ref.VClock([(1, 1)])}
    assert not py.entries[7][1].deferred and not py.deferred


def test_case_b_nested_duplicate_dot(oracle):
    m = og.case_b_map()
    py, _ = _both(oracle, [og.CASE_B_OP], m)
    ec, o = py.entries[7]
    assert o.clock.get(2) == 9 and o.entries[4] == crdts_ref.VClock([(2, 9)])  # the nested add was skipped
    assert ec.get(2) == 0 and py.clock.get(2) == 5  # witnessed, then the retired deferred remove took it
    assert list(py.deferred) == [crdts_ref.VClock([(1, 4)])]  # the deferred pass ran
    # without the deferred removes the entry clock keeps the dot
    m.deferred = {}
    py, _ = _both(oracle, [og.CASE_B_OP], m)
    assert py.entries[7][0].get(2) == 5 and py.entries[7][1].clock.get(2) == 9


def test_case_c_deferred_order_matters_and_oracle_takes_clock_order(oracle):
    py, cpp = _both(oracle, og.CASE_C)
    rev, _ = _both(oracle, og.CASE_C, order=lambda cs: crdts_ref.clock_order(cs)[::-1])
    assert len(py.entries[7][1].deferred) == 2 and len(rev.entries[7][1].deferred) == 1
    assert py != rev and cpp == py


def test_symbol_exported_and_null_ctx_is_einval():
    import crdts_hip
    from crdts_hip._lib import MapOrswotOpsC, lib

    assert "crdt_map_orswot_apply" in crdts_hip.EXPORTS
    S = crdts_hip.MapOrswotSlab.alloc(1, A, **og.caps(4))
    R = crdts_hip.MapOrswotSlab.alloc(1, A, **og.caps(8))
    s, r, o = S.cstruct(), R.cstruct(), MapOrswotOpsC()
    assert lib.crdt_map_orswot_apply(None, C.byref(s), C.byref(o), C.byref(r), 1, A, None) == crdts_hip.CRDT_EINVAL
    assert lib.crdt_map_orswot_apply(None, None, None, None, 0, A, None) == crdts_hip.CRDT_EINVAL


def test_map_orswot_ops_arrays_from_lists():
    import crdts_hip

    ends, kind, key, act, ctr, mem, cend, cact, cctr = crdts_hip.MapOrswotOps.arrays_from_lists(
        [[("up_add", 2, 5, 7, 99), ("nop",), ("up_rm", 1, 4, 8, 98, [(0, 1), (2, 5)])], [], [("rm", 9, [(1, 3)])]])
    assert ends.tolist() == [3, 3, 4] and kind.tolist() == [2, 0, 3, 1] and key.tolist() == [7, 0, 8, 9]
    assert act.tolist() == [2, 0, 1, 0] and ctr.tolist() == [5, 0, 4, 0] and mem.tolist() == [99, 0, 98, 0]
    assert cend.tolist() == [0, 0, 2, 3] and cact.tolist() == [0, 2, 1] and cctr.tolist() == [1, 5, 3]

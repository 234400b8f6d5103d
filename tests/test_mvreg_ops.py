"""MVReg op path, host side: the packing of MVRegOps (crdt_mvreg_ops), the
reference's op-side MVReg KATs (test/mvreg.rs:12-33, :60-79, :105-118) as op
scripts on the Python restatement, and the coverage of the seeded op generator
the GPU parity tests draw from (tests/mvreg_opgen.py)."""
import numpy as np
import pytest

import mvreg_opgen as mo


def test_mvreg_ops_packing():
    import crdts_hip

    per_obj = [[([(0, 1), (3, 2)], 7), ([], 8)],   # an empty clock between two objects' pairs
               [],                                  # no ops
               [([(2, 5)], 9)]]
    ends, val, cend, cact, cctr = crdts_hip.MVRegOps.arrays_from_lists(per_obj)
    assert ends.dtype == np.uint64 and ends.tolist() == [2, 2, 3]
    assert val.dtype == np.uint64 and val.tolist() == [7, 8, 9]
    assert cend.dtype == np.uint64 and cend.tolist() == [2, 2, 3]
    assert cact.dtype == np.uint32 and cact.tolist() == [0, 3, 2]
    assert cctr.dtype == np.uint64 and cctr.tolist() == [1, 2, 5]
    # all-empty op lists, and no objects at all
    for lists in ([[], [], []], []):
        ends, val, cend, cact, cctr = crdts_hip.MVRegOps.arrays_from_lists(lists)
        assert ends.tolist() == [0] * len(lists) and val.size == cend.size == cact.size == cctr.size == 0
    # only empty clocks: ops but no pairs
    ends, val, cend, cact, cctr = crdts_hip.MVRegOps.arrays_from_lists([[([], 1), ([], 2)]])
    assert ends.tolist() == [2] and cend.tolist() == [0, 0] and cact.size == 0


@pytest.mark.parametrize("pairs", [[(2, 1), (1, 1)], [(2, 1), (2, 2)], [(1, 0)]],
                         ids=["descending", "equal", "zero_counter"])
def test_mvreg_ops_rejects_noncanonical_clock(pairs):
    import crdts_hip

    with pytest.raises(ValueError):
        crdts_hip.MVRegOps.arrays_from_lists([[([(0, 1)], 1)], [(pairs, 2)]])


def test_mvreg_ops_cstruct_layout():
    """crdt_mvreg_ops: five pointers and two size_t, in the header's order."""
    import ctypes as C

    from crdts_hip._lib import MVRegOpsC

    assert [f for f, _ in MVRegOpsC._fields_] == ["obj_end", "val", "clk_end", "clk_act", "clk_ctr", "n_ops", "n_clk"]
    assert C.sizeof(MVRegOpsC) == 5 * C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_size_t)


KATS = mo.load_kats()


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_mvreg_op_kat_python(case):
    applies = mo.run_kat(case, mo.PyBackend())
    assert applies == sum(st[0] == "apply" for st in case["steps"]) > 0


def test_mvreg_op_kat_names():
    """Every known-answer test of test/mvreg.rs (:12-118): the four op-side
    ones, then the two that go through merge (:36-57 and :82-103; on the
    oracle's slabs they are tests/test_mvreg.py's too)."""
    assert [c["name"] for c in KATS] == ["test_apply", "test_set_should_not_mutate_reg",
                                        "test_concurrent_update_with_same_value_dont_collapse_on_apply",
                                        "test_op_commute_quickcheck1",
                                        "test_concurrent_update_with_same_value_dont_collapse_on_merge",
                                        "test_multi_val"]
    assert [sum(st[0] == "merge" for st in c["steps"]) for c in KATS] == [0, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("A,cap,hi", [(8, 4, 3), (16, 8, 2), (5, 16, 2), (1, 4, 3)])
def test_mvreg_opgen_covers_every_outcome(A, cap, hi):
    """Every outcome class of a Put occurs: add without / with a drop, skip
    without / with a drop (a Put that drops a value and is still not added),
    empty clock; and the final sizes spread."""
    b = mo.gen_batch(0x5EED + A, 2000, A, cap, hi, min_ops=8, max_ops=8)
    print(b["classes"], "peak", b["peak"])
    for c in mo.CLASSES:
        assert b["classes"][c] > 0, (c, b["classes"])
    assert sum(b["classes"].values()) == 2000 * 8
    sizes = {len(r.vals) for r in b["regs"]}
    # (one actor: all clocks are comparable, a register holds one value after any non-empty Put)
    assert len(sizes) >= 4 or A == 1, sizes
    assert b["peak"] <= cap + 8
    # the rendering round-trips, rows as given
    S = mo.slab(b["regs0"], cap, A)
    assert mo.setlike(*S) == mo.setlike(*mo.slab(mo.regs_of(*S), cap, A))
    assert (S[1][np.arange(cap)[None, :] >= S[0][:, None]] == 0).all()

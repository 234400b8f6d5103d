"""The run batches of the CSR clock suite (tests/clock_rungen.py) earn their
place without a GPU: the dict references, oracle/crdts_ref.py::VClock and the
C++ oracle agree on them, a census states the tiers and placements they hold,
and every deliberately wrong walk changes at least FLOOR objects of every
batch of its operation (both orientations for the merge) — while a signed
counter compare, and on the filter and apply batches a compare of the low
words, pass on the inputs of the older tests."""
import numpy as np
import pytest

import clock_rungen as cr
from mvreg_opgen import crdts_ref

FLOOR = 20
TABLE = {}


def _csr(runs):
    lens = np.array([len(r) for r in runs], np.uint32)
    off = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    return (off, lens, np.array([a for r in runs for a, _ in r], np.uint32),
            np.array([c for r in runs for _, c in r], np.uint64))


def test_references_agree(oracle):
    S, O = cr.pair_batch()
    for i, (s, o) in enumerate(zip(S, O)):
        v = crdts_ref.VClock(dict(s))
        v.merge(crdts_ref.VClock(dict(o)))
        assert cr.merge_dict(s, o) == list(v.canonical()) == cr.ref_merge(s, o), i
        for op in ("truncate", "subtract", "intersection"):
            v, w = crdts_ref.VClock(dict(s)), crdts_ref.VClock(dict(o))
            got = v.intersection(w) if op == "intersection" else (getattr(v, op)(w), v)[1]
            assert cr.filter_dict(op, s, o) == list(got.canonical()) == cr.ref_filter(op, s, o), (op, i)
        if i % 9 == 0 and len(s) + len(o) < 200:
            for op in ("merge", "subtract", "intersection"):
                exp = cr.merge_dict(s, o) if op == "merge" else cr.filter_dict(op, s, o)
                assert oracle.vclock_binop(op, list(s), list(o)) == exp, (op, i)
    cs, co = _csr(S), _csr(O)
    off, ln, act, ctr = oracle.vclock_csr_merge(cs, co)
    assert (off == cs[0] + co[0]).all()
    for i, (s, o) in enumerate(zip(S, O)):
        b = int(off[i])
        assert list(zip(act[b:b + ln[i]].tolist(), ctr[b:b + ln[i]].tolist())) == cr.merge_dict(s, o), i
    for s, p in zip(*cr.apply_batch()):
        v = crdts_ref.VClock(dict(s))
        for d in p:
            v.apply(d)
        assert cr.apply_dict(s, p) == list(v.canonical()) == cr.ref_apply(s, p)
    for s in cr.value_batch():
        g = crdts_ref.GCounter()
        g.inner = crdts_ref.VClock(dict(s))
        assert g.value() == cr.value_of(s) == cr.ref_value(s)
    for s, q in zip(*cr.get_batch()):
        v = crdts_ref.VClock(dict(s))
        assert [v.get(x) for x in q] == [cr.ref_get(s, x) for x in q]


def test_census():
    """The tiers and placements each batch holds."""
    S, O = cr.pair_batch()
    assert all(list(s) == sorted(set(s)) and all(c > 0 for _, c in s) for s in S + O)  # canonical runs
    c = cr.placements(S, O)
    TABLE["census"] = c
    assert {(len(s), len(o)) for s, o in zip(S, O)} == {(a, b) for a in cr.LENGTHS for b in cr.LENGTHS}
    # of the 9 x 9 length pairs, three times each: 5 x 5 both in registers, 2 x 5 x 4 one long, 4 x 4 both long;
    # a shared actor at index 63 wherever both runs reach it (5 x 5), at index 64 likewise (4 x 4)
    assert (c["regs"], c["one_long"], c["both_long"]) == (75, 120, 48)
    assert c["idx0"] >= 150 and c["idx63"] == 75 and c["idx64"] == 48 and c["last"] >= 90
    assert min(c["below"], c["equal"], c["above"]) >= 1000 and min(c["absent_self"], c["absent_other"]) >= 1000
    assert c["straddle"] >= 120
    # the 54 runs of exactly 64 entries, a third in each region: at and above 2^31 from lane 0, astride it, below it
    assert (c["run64_high_lane0"], c["run64_straddle"], c["run64_high_lane63"]) == (18, 18, 36)
    acts = {a for s in S + O for a, _ in s}
    assert acts >= set(cr.SPECIAL)
    assert sum(a ^ 2**31 in acts for a in acts) >= 500  # partners that differ only in bit 31,
    assert sum((a ^ 0x8001) in acts or (a ^ 0x7FFF) in acts for a in acts) >= 500  # only in the low 16 bits
    ctrs = {x for s in S + O for _, x in s}
    assert {2**32 - 1, 2**32, 2**63 - 1, 2**63, cr.M64 - 1, cr.M64} <= ctrs
    # a register run of 64 with actors at or above 2^31 at lane 0 and at lane 63 (runs of one actor and of 64)
    assert any(len(s) == 1 and s[0][0] >= 2**31 for s in S + O)
    SA, P = cr.apply_batch()
    assert {(len(s), len(p)) for s, p in zip(SA, P)} >= {(a, b) for a in cr.SELF_LENGTHS for b in cr.DOT_COUNTS}
    stand = [len({a for a, c in p if c}) for p in P]
    assert sum(len(p) == 64 and k == 64 for p, k in zip(P, stand)) >= 5  # 64 standing dots
    assert sum(len(p) == 64 and k < 64 for p, k in zip(P, stand)) >= 5  # 64 dots with repeats
    assert sum(bool(p) and not any(c for _, c in p) for p in P) >= 5  # counter-0 dots only
    assert sum(any(a == 0 for a, _ in p) and any(a == cr.AMAX for a, _ in p) for p in P) >= 5
    SG, Q = cr.get_batch()
    assert {len(s) for s in SG} == {2**k + d for k in range(10) for d in (-1, 0, 1)}
    present = sum(x in dict(s) for s, q in zip(SG, Q) for x in q)
    assert present >= 100 and sum(len(q) for q in Q) - present >= 300
    vals = [sum(c for _, c in s) >> 64 for s in cr.value_batch()]
    assert vals.count(1) >= FLOOR and sum(v >= 2 for v in vals) >= FLOOR  # sums that wrap once, twice and more


def _batches(op):
    if op == "merge":
        S, O = cr.pair_batch()
        return {"S_O": (S, O), "O_S": (O, S)}
    if op in ("truncate", "subtract", "intersection"):
        return {"S_O": cr.pair_batch()}
    return {"apply": {"dots": cr.apply_batch()}, "value": {"runs": cr.value_batch()},
            "get": {"queries": cr.get_batch()}}[op]


@pytest.mark.parametrize("op", sorted(cr.MUTANTS))
def test_wrong_walks_differ(op):
    """Every mutant of the operation changes >= FLOOR objects of each of its
    batches. One exemption: the intersection tests counters for equality, and
    reading both as signed keeps equal what is equal."""
    for mutant, knobs in cr.MUTANTS[op].items():
        for bname, batch in _batches(op).items():
            d = cr.differs(op, batch, knobs)
            TABLE[(op, bname, mutant)] = d
            if (op, mutant) == ("intersection", "counter_compare_signed"):
                assert d == 0
            else:
                assert d >= FLOOR, (op, bname, mutant, d)


def test_wrong_walks_table():
    """`-s -k wrong` prints what every mutant changes (objects)."""
    for key, d in TABLE.items():
        print(key, d)


# ---------------------------------------------- what the older inputs cannot see
def _runs(csr):
    off, ln, act, ctr = csr
    return [list(zip(act[o:o + n].tolist(), ctr[o:o + n].tolist())) for o, n in zip(off.tolist(), ln.tolist())]


def test_old_style_inputs_cannot_see_the_compare_mutants():
    """generate_clocks_csr draws its counters below 2^40 and the filter batch
    of tests/test_gpu_clock_ops.py below 2^62 (one two-entry pair apart, whose
    low words order as the counters do): a signed compare is the unsigned one
    there, and the filter batch's shared counters are one apart inside a low
    word, so a compare of the low words passes too. The apply lists are not
    blind to either compare (OLD_SEEN): the counts are upper bounds."""
    import crdts_hip
    from test_gpu_clock_ops import _apply_lists, _filter_batch

    s, o = crdts_hip.generate_clocks_csr(3000, seed=11)
    assert int(max(s[3].max(), o[3].max())) < 2**63
    pairs = list(zip(_runs(s), _runs(o)))
    assert cr.differs("merge", tuple(zip(*pairs)), dict(compare="signed")) == 0
    A, B = _filter_batch(np.random.default_rng(5))
    A, B = [sorted(a.items()) for a in A], [sorted(b.items()) for b in B]
    seen = {}
    for op in ("merge", "truncate", "subtract", "intersection"):
        for compare in ("signed", "low32"):
            seen[(op, compare)] = cr.differs(op, (A, B), dict(compare=compare))
    S, P = _apply_lists(np.random.default_rng(9))
    S = [sorted(x.items()) for x in S]
    for compare in ("signed", "low32"):
        seen[("apply", compare)] = cr.differs("apply", (S, P), dict(compare=compare))
    TABLE["old inputs"] = seen
    assert all(v <= OLD_SEEN.get(k, 0) for k, v in seen.items()), seen


# Objects of the older batches on which a wrong compare does show, measured (upper bounds). The filter batch
# and generate_clocks_csr see neither compare. The apply lists do see them, in 16 and 18 of their 36 objects:
# a fifth of their fresh dots carry 2^64 - 1, which a signed compare reads as -1, and a repeated actor draws
# an independent 62-bit counter, whose low word orders at random against the one before.
OLD_SEEN = {("apply", "signed"): 16, ("apply", "low32"): 18}

"""CPU proof for tests/test_gpu_map_edges.py: the lifted Map batches of
tests/map_edge_cases.py are what the oracle says they are, and they tell a
right Map kernel from the wrong ones of tests/map_lift.py.

- Equivariance: oracle(lift(S), lift(O)) == lift(oracle(S, O)), exact, for the
  three value kinds; merge in both orientations, truncate with the clock under
  the same lift, apply with the ops lifted; for the Python restatement and,
  where the entry point has one, the C++ oracle (which pins both 64-bit clean).
- Mutant floors: every wrong VClock comparison and every wrong key walk changes
  at least FLOOR objects of every merge batch, in both orientations.
- The gap: on the same batches unlifted, the low-32 and the signed compare
  agree with the right merge on at least 99 % of the objects.
- Census: every batch shows each key class and each way of deciding CLOCK
  ORDER on at least FLOOR objects, per orientation.
- Tiers: every batch of tests/map_tiergen.py holds FLOOR objects of each
  launch tier it is there for, and commutes with its lift."""
import collections

import numpy as np
import pytest

import map_edge_cases as mc
import map_lift as ml
import map_tiergen as mt
import map_truncgen as tg

FLOOR = mc.FLOOR
KINDS = mc.KINDS
WIDTHS = (16, 100)


def _merged(x, y):
    r = x.clone()
    r.merge(y)
    return r


def _sides(case, flip):
    return [(y, x) if flip else (x, y) for x, y in case["pairs"]], [(y, x) if flip else (x, y) for x, y in case["base"]]


# ------------------------------------------------------------------ the two forms of a lift agree
@pytest.mark.parametrize("kind", KINDS)
def test_slab_form_equals_object_form(kind):
    """lift_slab on the packed generated states gives the rows that packing
    the lifted objects gives; the identity lift gives the generated rows back."""
    c = mc.merge_case(kind, 16)
    base = mc.pack(kind, [p[0] for p in c["base"]], 16, c["caps"])
    assert mc.rows_differ(kind, ml.lift_slab(kind, base, c["lifts"]), c["S"]).size == 0
    assert mc.rows_differ(kind, mc.merge_case(kind, 16, lifted=False)["S"], base).size == 0
    assert mc.rows_differ(kind, c["S"], base).size > 0.9 * len(c["base"])
    t = mc.truncate_case(kind, 16)
    assert np.array_equal(ml.lift_clock_rows(tg.clock_rows(t["base_clocks"], 16), t["lifts"]), t["rows"])


@pytest.mark.parametrize("A", mc.MERGE_WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_merge_batches_hold_what_the_gpu_tests_need(kind, A):
    mc.assert_merge_batch(kind, A)


# ------------------------------------------------------------------ equivariance
@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_merge_commutes_with_the_lift(kind, A):
    c = mc.merge_case(kind, A)
    for flip, exp in ((False, c["SO"]), (True, c["OS"])):
        pairs, base = _sides(c, flip)
        rows = mc.unpack(kind, exp)
        for i, ((x, y), (bx, by), f) in enumerate(zip(pairs, base, c["lifts"])):
            want = ml.lift_map(_merged(bx, by), f)
            assert _merged(x, y) == want, (kind, A, flip, i)
            assert rows[i] == want, (kind, A, flip, i, "the entry point's oracle")
    if kind == "nested":  # the C++ restatement of the nested merge too
        import oracle_ffi

        assert mc.rows_differ(kind, oracle_ffi.map_map_merge(c["S"], c["O"], A), c["SO"]).size == 0
        assert mc.rows_differ(kind, oracle_ffi.map_map_merge(c["O"], c["S"], A), c["OS"]).size == 0


@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_truncate_commutes_with_the_lift(kind, A):
    c = mc.truncate_case(kind, A)
    rows = mc.unpack(kind, c["E"])
    changed = 0
    for i, (m, T, bm, bT, f) in enumerate(zip(c["states"], c["clocks"], c["base"], c["base_clocks"], c["lifts"])):
        want = ml.lift_map(tg.truncated(bm, bT), f)
        assert rows[i] == want, (kind, A, i)
        changed += want != m
    assert changed > 0.6 * len(rows)


@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_apply_commutes_with_the_lift(kind, A):
    c = mc.apply_case(kind, A)
    rows, starts = mc.unpack(kind, c["E"]), mc.unpack(kind, c["S"])
    for i, ((bs, _, bops), f) in enumerate(zip(c["base"], c["lifts"])):
        assert starts[i] == c["starts"][i], (kind, A, i, "start row")
        want = ml.lift_map(mc.replay(kind, bs, bops), f)
        assert mc.replay(kind, c["starts"][i], c["ops"][i]) == want, (kind, A, i)
        assert rows[i] == want, (kind, A, i, "the entry point's oracle")
    assert sum(r != s for r, s in zip(rows, starts)) > 0.7 * len(rows)


@pytest.mark.parametrize("name", list(mt.TIER_BATCHES))
def test_tier_batches(name):
    """Every tier batch holds FLOOR objects of each tier it is there for, in
    both orientations, and the entry point's oracle on the lifted pair gives
    the lift of the restatement's merge of the pair as built."""
    c = mt.tier_case(name)
    got = mt.assert_tiers(name)
    names = [k for w in mt.EXPECT[name] for k in (w.split("|") if isinstance(w, str) else [w])]
    print(f"\n{name}: " + ", ".join(f"{k} {got[0][k]}" for k in names))
    for flip, exp in ((False, c["SO"]), (True, c["OS"])):
        pairs, base = _sides(c, flip)
        rows = mc.unpack(c["kind"], exp)
        for i, ((bx, by), f) in enumerate(zip(base, c["lifts"])):
            assert rows[i] == ml.lift_map(_merged(bx, by), f), (name, flip, i)


# ------------------------------------------------------------------ wrong comparisons
_RIGHT = {}


def _changed_by(case, knob, flip, lifted=True):
    pairs, base = _sides(case, flip)
    use = pairs if lifted else base
    right = _RIGHT.setdefault((id(case), flip, lifted), [_merged(x, y) for x, y in use])  # the unpatched merges, once
    return sum(ml.changed(knob, lambda x=x, y=y: _merged(x, y), r) for (x, y), r in zip(use, right))


@pytest.mark.parametrize("knob", ml.VCLOCK_MUTANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_wrong_vclock_compare_changes_the_answers(kind, knob):
    """(high_slot_blind on the 100-actor batch: at 16 actors it is no mutant)"""
    c = mc.merge_case(kind, 100 if knob == "high_slot_blind" else 16)
    got = [_changed_by(c, knob, flip) for flip in (False, True)]
    print(f"\n{kind:7s} {knob:30s} self⊔other {got[0]:4d}  other⊔self {got[1]:4d}  of {len(c['pairs'])}")
    assert min(got) >= FLOOR, (kind, knob, got)


@pytest.mark.parametrize("knob", ml.KEY_MUTANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_wrong_key_walk_changes_the_answers(kind, knob):
    c = mc.merge_case(kind, 16)
    got = []
    for flip in (False, True):
        pairs, _ = _sides(c, flip)
        got.append(sum(ml.key_walk(sorted(x.entries), sorted(y.entries), knob)
                       != ml.key_walk(sorted(x.entries), sorted(y.entries)) for x, y in pairs))
    print(f"\n{kind:7s} {knob:30s} self⊔other {got[0]:4d}  other⊔self {got[1]:4d}  of {len(c['pairs'])}")
    assert min(got) >= FLOOR, (kind, knob, got)


def test_key_walk_is_the_sorted_union():
    c = mc.merge_case("orswot", 16)
    for x, y in c["pairs"]:
        ks, ko = sorted(x.entries), sorted(y.entries)
        assert ml.key_walk(ks, ko) == [(k, k in x.entries, k in y.entries) for k in sorted(set(ks) | set(ko))]


@pytest.mark.parametrize("knob", ["counter_compare_low32", "counter_compare_signed"])
@pytest.mark.parametrize("kind", KINDS)
def test_old_style_inputs_cannot_see_the_compare_mutants(kind, knob):
    """The gap this suite closes: on the generated batches as they are, a merge
    that compares 32 bits or compares signed agrees on at least 99 % of the objects."""
    c = mc.merge_case(kind, 16)
    for flip in (False, True):
        assert _changed_by(c, knob, flip, lifted=False) <= len(c["base"]) // 100, (kind, knob, flip)


# ------------------------------------------------------------------ census
KEY_CLASSES = ("zero", "all_ones", "low_word_pair", "high_word_pair", "around_2_63")


def _dclock_rows(kind, slab):
    a = slab.a
    return [a["dclock"][i, :int(a["n_def"][i])] for i in range(int(a["n_keys"].shape[0]))]


@pytest.mark.parametrize("kind", KINDS)
def test_census_of_the_merge_batches(kind):
    """Keys: every class on at least FLOOR objects, on either side. CLOCK
    ORDER of the output's deferred list: the high-word and low-word decisions
    at 16 actors; actors >= 64 and the prefix rule against the lane's other
    slot at 100."""
    c = mc.merge_case(kind, 16)
    keys = collections.Counter()
    for x, y in c["pairs"]:
        for cl in ml.key_census(sorted(x.entries)) | ml.key_census(sorted(y.entries)):
            keys[cl] += 1
    order = {(A, o): collections.Counter(cl for rows in _dclock_rows(kind, mc.merge_case(kind, A)[o])
                                         for cl in ml.clock_order_census(rows)) for A in WIDTHS for o in ("SO", "OS")}
    print(f"\n{kind}: keys {dict(keys)} order {({k: dict(v) for k, v in order.items()})}")
    assert all(keys[cl] >= FLOOR for cl in KEY_CLASSES), keys
    for o in ("SO", "OS"):
        assert all(order[16, o][cl] >= FLOOR for cl in ("high_word", "low_word")), order
        assert all(order[100, o][cl] >= FLOOR for cl in ml.ORDER_CLASSES), order


@pytest.mark.parametrize("kind", KINDS)
def test_every_edge_counter_and_image_kind_occurs(kind):
    for case in (mc.merge_case(kind, 16), mc.truncate_case(kind, 16), mc.apply_case(kind, 16)):
        kinds = collections.Counter(k for f in case["lifts"] for k in f.kinds["ctr"].values())
        assert all(kinds[k] >= FLOOR for k in ml.CTR_KINDS), kinds
        ctrs = {v for f in case["lifts"] for t in f.c.values() for v in t.values()}
        assert set(ml.EDGE_TOP) <= ctrs
        assert all(sum(f.kinds["key"] == k for f in case["lifts"]) >= FLOOR for k in set(ml.KEY_KINDS))
